"""Mesh -> point cloud with normals on the device (csrc/mesh.hip, dataprocess/mesh2pc_open3d.py, metrics.estimate_normals):
sampling and voxelisation bit for bit against the numpy restatement (tests/_mesh_ref.py), the neighbour sets and integer
covariances exactly, the normals against np.linalg.eigh, the degenerate rules, geometry checks, the CLI into
generate_dataset and eval's --estimate_normals."""
import configparser
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _mesh_ref as ref                                                  # noqa: E402
from pcgcv1_amd import _lib, metrics, synthetic                          # noqa: E402
from pcgcv1_amd.dataprocess import inout_points as iop                   # noqa: E402
from pcgcv1_amd.dataprocess import mesh2pc_open3d as m2p                 # noqa: E402

MESHES = {"icosphere": ref.icosphere, "torus": ref.torus, "quad_soup": ref.quad_soup}


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    _lib.require_gpu()


@pytest.mark.parametrize("mesh", sorted(MESHES))
def test_sample_and_voxelize_bit_exact(mesh):
    v, t = MESHES[mesh]()
    cdf = m2p.triangle_area_cdf(v, t)
    rot = m2p.get_rotate_matrix(11)
    for n in (1, 1000, 400000):
        for r in (None, rot):
            seed = 1234567 + n
            got = m2p.sample_points_uniformly(v, t, n, seed, r, cdf=cdf)
            want = ref.sample(v, t, n, seed, r)
            assert got.shape == (n, 3) and np.array_equal(_bits(got), _bits(want)), (mesh, n, r is None)
            for res in (255, 1023, 2047, 4095):               # 4095: the top of the range, a grid of 2^36 cells
                q = m2p.voxelize(got, res)
                assert q.dtype == np.int32 and np.array_equal(q, ref.voxelize(want, res)), (mesh, n, res)
    if mesh == "quad_soup":                                  # zero-area triangles are never sampled
        p = m2p.sample_points_uniformly(v, t, 20000, 9, cdf=cdf)
        tri = np.searchsorted(cdf, ref.uniforms(9, 20000)[0] * cdf[-1], side="right")
        area = np.diff(np.concatenate([[0.0], cdf]))
        assert (area[tri] > 0).all() and np.isfinite(p).all()


def test_sampler_draws_and_stream():
    u = ref.uniforms(77, 100000)
    assert (u >= 0).all() and (u < 1).all() and abs(u.mean() - 0.5) < 0.01
    v, t = ref.box()
    a = m2p.sample_points_uniformly(v, t, 5000, 77)
    b = m2p.sample_points_uniformly(v, t, 5000, 77)
    assert np.array_equal(_bits(a), _bits(b))
    assert not np.array_equal(a, m2p.sample_points_uniformly(v, t, 5000, 78))


def _check_normals(points, radius=10, max_nn=20):
    nrm, cov, k = metrics.estimate_normals(points, radius, max_nn, return_cov=True)
    C, K = ref.neighbour_cov(points, radius, max_nn)
    assert np.array_equal(k, K) and np.array_equal(cov, C)
    assert nrm.dtype == np.float32 and nrm.shape == (len(points), 3)
    want, lam, kind = ref.normals_from_cov(C, K)
    g = nrm.astype(np.float64)
    g /= np.linalg.norm(g, axis=1, keepdims=True)
    assert np.allclose(np.linalg.norm(nrm.astype(np.float64), axis=1), 1.0, atol=1e-6)
    eig = kind == 0
    gap = np.zeros(len(K))
    gap[eig] = (lam[eig, 1] - lam[eig, 0]) / np.maximum(lam[eig, 2], 1e-300)
    sep = eig & (gap > 1e-9)
    assert ((g[sep] * want[sep]).sum(1) >= 1 - 1e-9).all()
    rest = eig & ~sep
    if rest.any():
        Cf = ref.full(C[rest]).astype(np.float64)
        quad = np.einsum("ni,nij,nj->n", g[rest], Cf, g[rest])
        assert (quad <= lam[rest, 0] + 1e-9 * lam[rest, 2]).all()
    other = ~eig
    assert np.allclose(g[other], want[other], atol=1e-6)
    return nrm, kind


def test_normals_against_restatement_mesh_outputs():
    v, t = ref.torus()
    p = m2p.sample_points_uniformly(v, t, 400000, 5, m2p.get_rotate_matrix(5))
    pts = m2p.voxelize(p, 255)
    _check_normals(pts)
    v, t = ref.quad_soup()
    pts = m2p.voxelize(m2p.sample_points_uniformly(v, t, 30000, 6), 255)
    _check_normals(pts)


def test_normals_against_restatement_synthetic_cloud():
    pts = synthetic.make_cloud(seed=21, res=256)
    pts = np.concatenate([pts, pts[:500]])                   # duplicates share their cell's normal
    nrm, _ = _check_normals(pts)
    assert np.array_equal(nrm[-500:], nrm[:500])
    _check_normals(pts[:3000], radius=4.5, max_nn=7)         # sparse: most searches run to the end of a short table


def test_normals_degenerate_rules():
    lone = np.array([[5, 5, 5], [40, 40, 40], [41, 40, 40], [80, 0, 3]], np.int32)   # K = 1, 2, 2, 1
    nrm, cov, k = metrics.estimate_normals(lone, return_cov=True)
    assert np.array_equal(k, [1, 2, 2, 1]) and np.array_equal(nrm, np.tile(np.float32([0, 0, 1]), (4, 1)))
    line = np.array([[3 + i, 7 + 2 * i, 9] for i in range(8)], np.int32)            # direction (1, 2, 0): j = z
    nrm = metrics.estimate_normals(line)
    assert np.allclose(nrm, np.float32([2, -1, 0]) / np.sqrt(5), atol=1e-7)
    xline = np.array([[i, 4, 4] for i in range(3, 12)], np.int32)                   # direction x: y, z tie -> j = y
    assert np.array_equal(metrics.estimate_normals(xline), np.tile(np.float32([0, 0, 1]), (9, 1)))
    zline = np.array([[2, 2, 20 - i] for i in range(6)], np.int32)                  # direction z: j = x -> (0, 1, 0) after sign
    assert np.array_equal(metrics.estimate_normals(zline), np.tile(np.float32([0, 1, 0]), (6, 1)))
    _check_normals(np.concatenate([lone, line, xline + [0, 30, 0]]))


def test_normals_geometry():
    g = np.arange(40)
    xx, yy = np.meshgrid(g, g, indexing="ij")
    plane = np.stack([xx.ravel(), yy.ravel(), np.full(xx.size, 7)], -1).astype(np.int32)
    assert np.array_equal(metrics.estimate_normals(plane), np.tile(np.float32([0, 0, 1]), (len(plane), 1)))
    assert np.array_equal(metrics.estimate_normals(plane[:, [2, 0, 1]]), np.tile(np.float32([1, 0, 0]), (len(plane), 1)))
    assert np.array_equal(metrics.estimate_normals(plane[:, [0, 2, 1]]), np.tile(np.float32([0, 1, 0]), (len(plane), 1)))
    v, t = ref.icosphere(level=4, radius=100.0)
    p = m2p.sample_points_uniformly(v, t, 600000, 3) + 128.0
    pts = np.unique(np.rint(p).astype(np.int32), axis=0)
    nrm = metrics.estimate_normals(pts)
    r = pts - 128.0
    r /= np.linalg.norm(r, axis=1, keepdims=True)
    assert (np.abs((nrm * r).sum(1)) > 0.95).mean() >= 0.99


def _write_meshes(d):
    os.makedirs(d / "a", exist_ok=True)
    v, t = ref.icosphere(level=3)
    with open(d / "a" / "sphere.off", "w") as f:
        f.write("OFF%d %d 0\n" % (len(v), len(t)))
        f.writelines("%r %r %r\n" % tuple(p) for p in v.tolist())
        f.writelines("3 %d %d %d\n" % tuple(q) for q in t.tolist())
    v, t = ref.torus()
    with open(d / "ring.obj", "w") as f:
        f.write("# torus\n")
        f.writelines("v %r %r %r\n" % tuple(p) for p in v.tolist())
        f.writelines("f %d/1 %d/1 %d/1\n" % tuple(q) for q in (t + 1).tolist())


def test_cli_into_generate_dataset_deterministic(tmp_path):
    from pcgcv1_amd import generate_dataset
    _write_meshes(tmp_path / "meshes")
    outs = []
    for run in ("o1", "o2"):
        m2p.main(["--input_rootdir", str(tmp_path / "meshes"), "--output_rootdir", str(tmp_path / run), "--n_testdata", "2",
                  "--n_points", "50000", "--resolution", "255", "--seed", "4"])
        outs.append(sorted(os.listdir(tmp_path / run)))
    assert outs[0] == outs[1] and len(outs[0]) == 2 and all(f.endswith(".ply") for f in outs[0])
    for f in outs[0]:
        assert (tmp_path / "o1" / f).read_bytes() == (tmp_path / "o2" / f).read_bytes()
        pts, nrm = iop.load_ply_normals(str(tmp_path / "o1" / f))
        assert nrm is not None and len(pts) > 1000 and pts.min() >= 0 and pts.max() == 255
        assert np.allclose(np.linalg.norm(nrm, axis=1), 1, atol=1e-5)
    # the function form returns what it writes
    seed = 4 * 1000003
    pts, nrm = m2p.mesh2pc(str(tmp_path / "meshes" / "ring.obj"), str(tmp_path / "r.ply"), 50000, 255, seed=seed)
    gp, gn = iop.load_ply_normals(str(tmp_path / "r.ply"))
    assert np.array_equal(gp, pts) and np.allclose(gn, nrm, atol=6e-7)
    assert np.array_equal(nrm, metrics.estimate_normals(pts))
    written = generate_dataset.generate_dataset(str(tmp_path / "o1"), str(tmp_path / "cubes"), 1e6, cube_size=64, seed=0)
    assert len(written) > 0 and all(os.path.exists(w) for w in written)
    assert np.load(written[0]).dtype == np.uint8


def _normal_free_ply(path):
    pts = synthetic.make_cloud(seed=6, res=128, n_shells=3, rmin=0.2, rmax=0.4)
    iop.write_ply_data(str(path), pts)
    return pts


def test_eval_estimate_normals(tmp_path, monkeypatch):
    from pcgcv1_amd import eval as pe
    pts = _normal_free_ply(tmp_path / "bare_vox7.ply")
    assert iop.load_ply_normals(str(tmp_path / "bare_vox7.ply"))[1] is None
    body = "[DEFAULT]\ncube_size = 64\nmin_num = 20\n\n[R1]\nscale = 1.0\nckpt_dir = synthetic:7:sparse\n"
    recs = {}
    real = pe.postprocess_points

    def spy(*a):
        rec = real(*a)
        recs[a[5]] = rec
        return rec
    monkeypatch.setattr(pe, "postprocess_points", spy)
    ini = tmp_path / "on.ini"
    ini.write_text(body)
    rows = pe.eval(str(tmp_path / "bare_vox7.ply"), str(tmp_path / "res_on"), str(ini), 128, estimate_normals=True)
    row = rows[0]
    rec = np.unique(np.rint(recs[1.0]).astype(np.int32), axis=0)
    want = metrics.pc_error(pts, rec, metrics.estimate_normals(pts), 127)
    for key in want:
        assert row[key] == want[key], key
    assert np.isfinite(row["optimal D2 PSNR"]) and np.isfinite(row["mseF,PSNR (p2plane)"])
    cfg = configparser.ConfigParser()
    cfg.read(str(ini))
    assert cfg.has_option("R1", "rho_d2") and float(cfg.get("R1", "rho_d2")) == row["rho_d2"]
    # without the flag: no p2plane figures, NaN optimal D2, no rho_d2 written (as before)
    ini2 = tmp_path / "off.ini"
    ini2.write_text(body)
    row2 = pe.eval(str(tmp_path / "bare_vox7.ply"), str(tmp_path / "res_off"), str(ini2), 128)[0]
    assert not any("p2plane" in k for k in row2) and np.isnan(row2["optimal D2 PSNR"]) and row2["rho_d2"] == 1.0
    cfg2 = configparser.ConfigParser()
    cfg2.read(str(ini2))
    assert cfg2.has_option("R1", "rho_d1") and not cfg2.has_option("R1", "rho_d2")
    # and the flagged run reproduces itself
    ini3 = tmp_path / "again.ini"
    ini3.write_text(body)
    rows3 = pe.eval(str(tmp_path / "bare_vox7.ply"), str(tmp_path / "res_again"), str(ini3), 128, estimate_normals=True)
    assert rows3 == rows and ini3.read_text() == ini.read_text()


def test_ablation_cli_passes_the_flag(monkeypatch):
    from pcgcv1_amd import eval_ablation_studies as abl
    seen = {}

    def fake(input_file, *a, **k):
        seen[input_file] = k.get("estimate_normals")
        return []
    monkeypatch.setattr(abl.rd, "eval", fake)
    monkeypatch.setattr(abl.rd, "set_default_config", lambda *a, **k: (None, "cfg.ini"))
    abl.main(["--input", "x.ply", "--estimate_normals"])
    abl.main(["--input", "y.ply"])
    assert seen == {"x.ply": True, "y.ply": False}
