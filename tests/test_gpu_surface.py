"""The surface kernels (csrc/surface.hip through pcgcv1_amd/surface.py) against the rule in numpy (tests/_surface_ref.py): signs
and round counts equal, the lattice keys equal, the signed distance and the mesh vertices bit for bit, the triangles equal up to
their order and rotation; then the topology of what comes out, the errors, and a ply through the command line.

The normals are metrics.estimate_normals' (radius 10, 20 neighbours), unoriented as they come.  The reference of every shape
is computed once per module."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _surface_ref as ref                                               # noqa: E402
from pcgcv1_amd import _lib, metrics, surface                            # noqa: E402
from pcgcv1_amd.dataprocess import inout_points as iop                   # noqa: E402
from pcgcv1_amd.dataprocess import mesh2pc_open3d as m2p                 # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "surface_sphere5_normals.npz")
C5, R5 = (15.5, 15.5, 15.5), 10.3
C7, R7 = (63.5, 63.5, 63.5), 50.0


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    _lib.require_gpu()


def _points(name):
    if name == "sphere5":
        return ref.sphere(C5, R5), 5
    if name == "sphere7":
        return ref.sphere(C7, R7, n=1500000), 7
    if name == "torus":
        return ref.torus(), 5
    if name == "patch":
        return ref.paraboloid(), 5
    if name == "two":
        return np.unique(np.r_[ref.sphere((15.5, 15.5, 15.5), 9.0), ref.sphere((45.5, 40.5, 40.5), 11.0, seed=4)], axis=0), 6
    if name == "faces":                                                  # touches 0 and res - 1 on every axis
        return ref.sphere(C5, 15.5), 5
    raise KeyError(name)


SHAPES = ("sphere5", "sphere7", "torus", "patch", "two", "faces")


@functools.lru_cache(maxsize=None)
def shape(name):
    """(points in a random row order, bits, normals float32, the rule's (vertices, triangles, report) at R = 3)"""
    p, bits = _points(name)
    p = p[np.random.default_rng(len(p)).permutation(len(p))]
    assert p.min() >= 0 and p.max() < 1 << bits
    nr = metrics.estimate_normals(p)
    return p, bits, nr, ref.reconstruct(p, nr, bits, 3)


def test_shape_sizes():
    sizes = {name: len(_points(name)[0]) for name in SHAPES}
    assert 1200 < sizes["sphere5"] < 2100 and 30000 < sizes["sphere7"] < 50000 and sizes["patch"] < 700
    p, bits = _points("faces")
    assert p.min(0).tolist() == [0, 0, 0] and p.max(0).tolist() == [31, 31, 31]
    assert (32 + 3) ** 3 < 4096 * 32 < (128 + 2) ** 3                    # bits 5: one scan block; bits 7: several


# ---------------------------------------------------------------------------- orientation
@pytest.mark.parametrize("name", SHAPES)
def test_orient(name):
    p, bits, nr, (_, _, want) = shape(name)
    report = {}
    sign, rounds = surface.orient(p, nr, bits, report=report)
    assert sign.dtype == np.int8 and sign.shape == (len(p),)
    print("%s: %d voxels, %d rounds (the rule: %d), %d read-backs, %d components" % (
        name, len(p), rounds, want["rounds"], report["readbacks"], report["components"]))
    np.testing.assert_array_equal(sign, want["sign"])
    assert rounds == want["rounds"] > 3
    assert report["readbacks"] == 1 + -(-rounds // surface.ROUNDS_PER_READ)
    assert report["components"] == (2 if name == "two" else 1)
    again, rounds2 = surface.orient(p, nr, bits)
    assert again.tobytes() == sign.tobytes() and rounds2 == rounds
    centres = {"sphere5": [C5], "sphere7": [C7], "faces": [C5], "two": [(15.5, 15.5, 15.5), (45.5, 40.5, 40.5)]}.get(name)
    if centres:                                                          # every oriented normal points away from its centre
        c = np.array(centres)
        nearest = c[np.argmin(np.linalg.norm(p[:, None, :] - c[None], axis=2), axis=1)]
        out = (sign[:, None] * nr.astype(np.float64) * (p - nearest)).sum(1)
        assert (out > 0).all(), (int((out <= 0).sum()), len(p))


def test_orient_gap_and_thresholds():
    p, bits, nr, _ = shape("torus")
    for gap, tau in ((2, (0.9, 0.0)), (8, (0.9, 0.0)), (1, (0.0,)), (1, (0.99, 0.9, 0.5, 0.0)), (1, (0.5, 0.97, 0.0)),
                     (1, (0.95, 0.95, 0.0))):             # thresholds that rise, and that repeat
        want = ref.orient(p, nr, bits, gap=gap, tau=tau)
        sign, rounds = surface.orient(p, nr, bits, "propagate", gap, tau)
        np.testing.assert_array_equal(sign, want[0])
        assert rounds == want[1], (gap, tau)
    sign, rounds = surface.orient(p, nr, bits, "propagate:2")
    np.testing.assert_array_equal(sign, ref.orient(p, nr, bits, gap=2)[0])


def test_orient_rounds_do_not_depend_on_the_batch():
    p, bits, nr, (_, _, want) = shape("sphere5")
    pp, nn, key, _ = surface._validated(p, nr, bits)
    lat = surface._Lattice(pp, bits)
    seed, _ = surface._seeds(pp, key, bits, 1)
    for batch in (1, 7, 4096):
        sign, rounds, reads = lat.orient(nn, seed, 1, (0.9, 0.0), batch)
        np.testing.assert_array_equal(sign.cpu().numpy(), want["sign"])
        assert rounds == want["rounds"] and reads == 1 + -(-rounds // batch)


def test_view_given_and_one_voxel():
    p, bits, nr, _ = shape("patch")
    sign, rounds = surface.orient(p, nr, bits, "given")
    assert (sign == 1).all() and rounds == 0
    view = (15.5, 15.5, 200.0)
    sign, rounds = surface.orient(p, nr, bits, "view:15.5,15.5,200")
    np.testing.assert_array_equal(sign, ref.orient(p, nr, bits, "view", view=view)[0])
    assert rounds == 0 and (sign[:, None] * nr)[:, 2].min() > 0
    one, n1 = np.array([[3, 4, 5]], np.int32), np.array([[0, 0, 1]], np.float32)
    assert surface.orient(one, n1, 3) == (pytest.approx([1]), 0)
    v, t, report = surface.reconstruct(one, n1, 3)
    want_v, want_t, _ = ref.reconstruct(one, n1, 3)
    assert v.tobytes() == want_v.tobytes() and len(t) > 0
    np.testing.assert_array_equal(surface.canonical(t), ref.canonical(want_t))
    np.testing.assert_allclose(v[:, 2], 5.0, atol=1e-12)                 # the plane through the voxel's centre
    assert report["rounds"] == 0 and report["components"] == 1 and report["boundary_edges"] > 0
    for corner, bits in (([0, 0, 0], 1), ([1, 1, 1], 1), ([1, 0, 1], 1)):
        one = np.array([corner], np.int32)
        v, t, _ = surface.reconstruct(one, n1, bits)
        want_v, want_t, _ = ref.reconstruct(one, n1, bits)
        assert v.tobytes() == want_v.tobytes() and np.array_equal(surface.canonical(t), ref.canonical(want_t))


def test_64_bit_cell_indices():
    """bits = 11: 2^33 cells, the lattice keys beyond 2^33 and the edge ids beyond 2^35; one voxel at the far corner gives the
    mesh of one voxel anywhere, moved there"""
    corner = np.array([[2047, 2046, 2047]], np.int32)
    n1 = np.array([[0, 0, 1]], np.float32)
    keys, f = surface.implicit(corner, n1.astype(np.float64), 11)
    want_keys, want_f = ref.implicit(corner % 8, n1.astype(np.float64), 3)
    k = ref.vertex_of_key(want_keys, 3) + (corner - corner % 8)
    np.testing.assert_array_equal(keys, ref.vertex_keys(k, 11))
    assert keys.max() > 2 ** 33 and np.array_equal(f, want_f)
    v, t, _ = surface.reconstruct(corner, n1, 11)
    want_v, want_t, _ = ref.reconstruct(corner % 8, n1, 3)
    np.testing.assert_allclose(v - corner, want_v - corner % 8, rtol=0, atol=1e-9)
    np.testing.assert_array_equal(surface.canonical(t), ref.canonical(want_t))


# ---------------------------------------------------------------------------- the signed distance
@pytest.mark.parametrize("radius", [3, 5])
@pytest.mark.parametrize("name", SHAPES)
def test_implicit(name, radius):
    p, bits, nr, (_, _, want) = shape(name)
    N = ref.oriented(nr, want["sign"])
    keys, f = (want["vertex_keys"], want["f"]) if radius == 3 else ref.implicit(p, N, bits, radius)
    got_keys, got_f = surface.implicit(p, N, bits, radius)
    assert got_keys.dtype == np.int64 and got_f.dtype == np.float64
    np.testing.assert_array_equal(got_keys, keys)
    assert np.isfinite(got_f).all()
    diff = np.abs(got_f - f)
    print("%s R = %d: %d lattice vertices, max |f - rule| = %g" % (name, radius, len(f), diff.max()))
    assert np.array_equal(got_f, f), (int((got_f != f).sum()), float(diff.max()))


def test_implicit_at_the_largest_radius():
    p, bits, nr, (_, _, want) = shape("torus")
    N = ref.oriented(nr, want["sign"])
    keys, f = ref.implicit(p, N, bits, 8)
    got_keys, got_f = surface.implicit(p, N, bits, 8)
    assert np.array_equal(got_keys, keys) and np.array_equal(got_f, f)


# ---------------------------------------------------------------------------- the mesh
@pytest.mark.parametrize("name", SHAPES)
def test_reconstruct(name):
    p, bits, nr, (want_v, want_t, want) = shape(name)
    v, t, report = surface.reconstruct(p, nr, bits)
    assert v.dtype == np.float64 and t.dtype == np.int32 and t.shape[1] == 3
    print("%s: %s" % (name, surface.summary_line(report)))
    assert report["cells"] == want["cells"] and report["lattice_vertices"] == len(want["f"])
    assert v.shape == want_v.shape and v.tobytes() == want_v.tobytes()
    np.testing.assert_array_equal(surface.canonical(t), ref.canonical(want_t))
    assert (report["voxels"], report["rounds"], report["vertices"], report["triangles"]) == (len(p), want["rounds"], len(v), len(t))
    v2, t2, _ = surface.reconstruct(p, nr, bits)
    assert v2.tobytes() == v.tobytes() and t2.tobytes() == t.tobytes()
    # topology
    _, ucount, dmax = ref.edge_census(t)
    assert dmax == 1                                                     # every directed edge once: consistently wound
    loops, n_boundary = ref.boundary_loops(t)
    assert report["boundary_edges"] == n_boundary
    if name == "patch":
        assert loops == 1 and n_boundary > 50 and ref.euler(v, t) == 1 and (ucount <= 2).all()
    else:
        assert (ucount == 2).all() and loops == 0
        assert ref.euler(v, t) == {"torus": 0, "two": 4}.get(name, 2)
        assert ref.signed_volume(v, t) > 0
    if name == "faces":
        k = ref.vertex_of_key(want["vertex_keys"], bits)                 # the surface leaves the grid: cells and vertices below 0
        assert k.min(0).tolist() == [-2, -2, -2] and k.max(0).tolist() == [32, 32, 32] and v.min() < 0 and v.max() > 31


def _deviation(v, t):
    """the largest | |v - centre| - r | over the vertices and the relative error of the enclosed volume"""
    radial = float(np.abs(np.linalg.norm(v - np.array(C5), axis=1) - R5).max())
    ball = 4.0 / 3.0 * np.pi * R5 ** 3
    return radial, abs(ref.signed_volume(v, t) - ball) / ball


def test_sphere_against_the_analytic_sphere():
    """The bound is 1.5 times the reference's own deviation, computed here on the CPU from the committed normals of the bits-5
    sphere (tests/golden/surface_sphere5_normals.npz, written by estimate_normals on the GPU): the surface is smoothed and the
    shell one voxel thick, so no bound can be derived.  Measured, reference and device alike (the meshes are the same bytes):
    largest radial deviation 0.5431 voxels, volume off by 3.61 % of the ball's."""
    p, bits, nr, _ = shape("sphere5")
    gold = np.load(GOLDEN)
    order = np.lexsort((p[:, 2], p[:, 1], p[:, 0]))
    np.testing.assert_array_equal(gold["points"], p[order])
    np.testing.assert_array_equal(gold["normals"], nr[order])            # the kernel still estimates what the fixture holds
    want_v, want_t, _ = ref.reconstruct(gold["points"], gold["normals"], bits, 3)
    want = _deviation(want_v, want_t)
    v, t, _ = surface.reconstruct(p, nr, bits)
    got = _deviation(v, t)
    print("sphere5: radial deviation %.6g (the rule: %.6g), volume %.6g (the rule: %.6g)" % (got[0], want[0], got[1], want[1]))
    assert got[0] <= 1.5 * want[0] and got[1] <= 1.5 * want[1]
    assert want[0] < 1.0 and want[1] < 0.1                               # and the rule's own is a fraction of a voxel


# ---------------------------------------------------------------------------- errors
def test_python_refuses_what_the_rule_excludes():
    p, bits, nr, _ = shape("patch")
    bad = nr.copy()
    bad[17, 1] = np.nan
    with pytest.raises(ValueError, match="row 17.*not finite or not of unit length"):
        surface.reconstruct(p, bad, bits)
    bad = nr.copy()
    bad[5] *= 1.01
    with pytest.raises(ValueError, match="row 5.*unit length"):
        surface.orient(p, bad, bits)
    with pytest.raises(ValueError, match="duplicate"):
        surface.reconstruct(np.r_[p, p[3:4]], np.r_[nr, nr[3:4]], bits)
    out = p.copy()
    out[9, 2] = 32
    with pytest.raises(ValueError, match="row 9.*outside the grid"):
        surface.reconstruct(out, nr, bits)
    out[9, 2] = -1
    with pytest.raises(ValueError, match="row 9.*outside the grid"):
        surface.implicit(out, nr.astype(np.float64), bits)
    for radius in (2, 9):
        with pytest.raises(ValueError, match="radius"):
            surface.reconstruct(p, nr, bits, radius=radius)
        with pytest.raises(ValueError, match="radius"):
            surface.implicit(p, nr.astype(np.float64), bits, radius)
    for gap in (0, 9):
        with pytest.raises(ValueError, match="gap"):
            surface.orient(p, nr, bits, gap=gap)
        with pytest.raises(ValueError, match="gap"):
            surface.reconstruct(p, nr, bits, orient="propagate:%d" % gap)
    with pytest.raises(ValueError, match="last stage threshold"):
        surface.orient(p, nr, bits, tau=(0.9, 0.1))
    with pytest.raises(ValueError, match="bits"):
        surface.reconstruct(p, nr, 13)
    with pytest.raises(ValueError, match="points and .* normals"):
        surface.orient(p, nr[:-1], bits)


def test_bad_arguments_touch_nothing():
    lib = _lib.hip()
    sized = lib.pcgc_surface_workspace_bytes
    assert sized(0, 10) == 0 and sized(13, 10) == 0 and sized(5, 0) == 0 and sized(5, 2 ** 31) == 0
    assert sized(5, 1000) >= (2 * 32 ** 3 + 34 ** 3 + 2 * 35 ** 3) // 8 + 30 * 1000
    dev = _lib.require_gpu()
    p, bits, nr, _ = shape("patch")
    n = len(p)
    pp, nn = torch.from_numpy(p).to(dev), torch.from_numpy(nr).to(dev)
    seed = torch.zeros(n, dtype=torch.uint8, device=dev)
    ws = torch.full((int(sized(bits, n)),), 0x5A, dtype=torch.uint8, device=dev)
    sign = torch.full((n,), -7, dtype=torch.int8, device=dev)
    counts = torch.full((2,), -7, dtype=torch.int64, device=dev)
    keys = torch.full((100,), -7, dtype=torch.int64, device=dev)
    f = torch.full((100,), -7.0, dtype=torch.float64, device=dev)
    N = nn.double().contiguous()
    import ctypes
    rounds = ctypes.c_int32(-7)
    s = _lib.stream()

    def orient(gap=1, tau=(0.9, 0.0), batch=32, n=n, bits=bits, ws_bytes=ws.numel(), points=pp):
        tau_c = (ctypes.c_double * len(tau))(*tau)
        return lib.pcgc_surface_orient(_lib.dptr(points), _lib.dptr(nn), _lib.dptr(seed), n, bits, gap, ctypes.cast(tau_c, ctypes.c_void_p), len(tau),
                                       batch, _lib.dptr(sign), ctypes.cast(ctypes.byref(rounds), ctypes.c_void_p), None, _lib.dptr(ws), ws_bytes, s)
    for kw, what in ((dict(gap=0), b"gap"), (dict(gap=9), b"gap"), (dict(tau=(0.9, 0.1)), b"last stage threshold"), (dict(tau=(1.5, 0.0)), b"outside [0, 1]"),
                     (dict(batch=0), b"batch"), (dict(n=0), b"bad arguments"), (dict(bits=13), b"bad arguments"), (dict(points=None), b"bad arguments"),
                     (dict(ws_bytes=ws.numel() - 1), b"workspace too small")):
        assert orient(**kw) == -1, kw
        err = lib.pcgc_last_error()
        assert err.startswith(b"pcgc_surface_orient") and what in err, (kw, err)
    assert lib.pcgc_surface_lattice(_lib.dptr(pp), n, 0, _lib.dptr(counts), _lib.dptr(ws), ws.numel(), s) == -1
    assert lib.pcgc_surface_lattice(_lib.dptr(pp), n, bits, None, _lib.dptr(ws), ws.numel(), s) == -1
    for radius in (2, 9):
        assert lib.pcgc_surface_implicit(_lib.dptr(N), n, bits, radius, 100, _lib.dptr(keys), _lib.dptr(f), _lib.dptr(ws), ws.numel(), s) == -1
        assert b"radius" in lib.pcgc_last_error()
    assert lib.pcgc_surface_implicit(_lib.dptr(N), n, bits, 3, 100, _lib.dptr(keys), _lib.dptr(f), _lib.dptr(ws), 10, s) == -1
    assert lib.pcgc_surface_triangles(_lib.dptr(f), 100, n, bits, 0, None, None, _lib.dptr(ws), ws.numel(), s) == -1
    assert lib.pcgc_surface_mesh(None, 1, _lib.dptr(keys), 1, _lib.dptr(f), 100, n, bits, _lib.dptr(f), _lib.dptr(keys), _lib.dptr(ws), ws.numel(), s) == -1
    torch.cuda.synchronize()
    assert (sign == -7).all() and (counts == -7).all() and (keys == -7).all() and (f == -7.0).all() and (ws == 0x5A).all()
    assert rounds.value == -7
    # no seed at all: the rounds end at the last stage with an error, and sign is not written
    assert orient() == -1 and b"seed" in lib.pcgc_last_error()
    torch.cuda.synchronize()
    assert (sign == -7).all() and rounds.value == -7


# ---------------------------------------------------------------------------- end to end
def test_a_ply_through_the_command_line(tmp_path, monkeypatch, capsys):
    p, bits, nr, _ = shape("torus")
    monkeypatch.chdir(tmp_path)
    iop.write_ply_normals("torus.ply", p, nr)
    read_p, read_n = iop.load_ply_normals("torus.ply")
    np.testing.assert_array_equal(read_p, p)
    surface.main(["--input", "torus.ply", "--output", "torus.obj"])
    said = capsys.readouterr().out.splitlines()
    want_v, want_t, want = ref.reconstruct(read_p, read_n, bits, 3)
    assert said == ["surface: %d voxels, 1 components, %d rounds, %d vertices, %d triangles, 0 boundary edges" % (
        len(p), want["rounds"], len(want_v), len(want_t)), "wrote torus.obj"]
    v, t = m2p.read_triangle_mesh("torus.obj")
    assert v.tobytes() == want_v.tobytes()
    np.testing.assert_array_equal(surface.canonical(t), ref.canonical(want_t))
    # the mesh sampled and voxelised again lies on the cloud it came from, exactly as the rule's mesh does
    mse = []
    for vv, tt in ((v, t), (want_v, ref.canonical(want_t))):
        cloud = m2p.voxelize(m2p.sample_points_uniformly(vv, surface.canonical(tt), 200000, seed=1), 31)
        mse.append(metrics.d1_metrics(p, cloud, 31)["mseF      (p2point)"])
    print("D1 mse of the resampled mesh against the cloud: %g" % mse[0])
    assert mse[0] == mse[1] and mse[0] < 4.0
    # .off, another radius, estimated normals, a frame
    from pcgcv1_amd import ingest
    frame = ingest.Frame((1.0, -2.0, 0.5), 0.25, bits)
    ingest.write_frame("torus.frame", frame)
    surface.main(["--input", "torus.ply", "--output", "torus.off", "--radius", "4", "--estimate_normals", "--frame", "torus.frame",
                  "--orient", "propagate:2"])
    assert capsys.readouterr().out.splitlines()[-1] == "wrote torus.off"     # after this test's own D1 line and the summary
    v4, t4 = m2p.read_triangle_mesh("torus.off")
    w4, wt4, _ = ref.reconstruct(p, nr, bits, 4, gap=2)
    assert v4.tobytes() == ingest.apply_frame(w4, frame).tobytes()
    np.testing.assert_array_equal(surface.canonical(t4), ref.canonical(wt4))


def test_decompress_writes_a_mesh(tmp_path, monkeypatch, capsys):
    from pcgcv1_amd import test as cli
    p, bits, _, _ = shape("sphere5")
    monkeypatch.chdir(tmp_path)
    iop.write_ply_data("ball.ply", p)
    cli.main(["compress", "ball.ply", "ball", "--ckpt_dir=synthetic:0"])
    capsys.readouterr()
    cli.main(["decompress", "compressed/ball", "ball_rec.ply", "--ckpt_dir=synthetic:0", "--mesh", "ball.obj"])
    said = capsys.readouterr().out
    rec = iop.load_ply_data("ball_rec.ply")
    v, t = m2p.read_triangle_mesh("ball.obj")
    want_v, want_t, report = surface.reconstruct(rec)
    assert surface.summary_line(report) in said and "Mesh ball_rec.ply to ball.obj" in said
    assert v.tobytes() == want_v.tobytes() and np.array_equal(surface.canonical(t), surface.canonical(want_t)) and len(t) > 0
    with pytest.raises(SystemExit, match="--mesh belongs to decompress"):
        cli.main(["compress", "ball.ply", "ball", "--ckpt_dir=synthetic:0", "--mesh", "ball.obj"])
    with pytest.raises(SystemExit):
        cli.main(["decompress", "compressed/ball", "ball_rec.ply", "--ckpt_dir=synthetic:0", "--mesh", "ball.stl"])
