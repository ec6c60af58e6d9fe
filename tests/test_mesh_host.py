"""Host side of mesh -> point cloud (dataprocess/mesh2pc_open3d.py): the OFF / OBJ parser (pcgc_parse_mesh), the area
running sum (pcgc_mesh_area_cdf) bit for bit against its numpy restatement (tests/_mesh_ref.py), the seeded rotation and
the ply writer with normals.  No GPU needed."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _mesh_ref as ref                                                  # noqa: E402
from pcgcv1_amd.dataprocess import inout_points as iop                   # noqa: E402
from pcgcv1_amd.dataprocess import mesh2pc_open3d as m2p                 # noqa: E402


def test_parse_off_modelnet_header_quads_and_comments():
    # ModelNet40's first line carries the counts glued to the magic; a quad is fan-triangulated; a face line may carry colours
    text = ("OFF5 3 0\n"
            "0 0 0\n1 0 0\n1.5 1 0\n0 1 -2.25\n"
            "# a comment line\n"
            "3e-1 0.5 1e2\n"
            "4 0 1 2 3\n"
            "3 0 1 4 255 0 0\n"
            "\n"
            "5 0 1 2 3 4\n")
    v, t = m2p.parse_mesh(text, 0)
    assert v.dtype == np.float64 and t.dtype == np.int32
    assert np.array_equal(v, [[0, 0, 0], [1, 0, 0], [1.5, 1, 0], [0, 1, -2.25], [0.3, 0.5, 100.0]])
    assert np.array_equal(t, [[0, 1, 2], [0, 2, 3], [0, 1, 4], [0, 1, 2], [0, 2, 3], [0, 3, 4]])


def test_parse_off_counts_on_their_own_line():
    v, t = m2p.parse_mesh("OFF\n# made by hand\n3 1 3\n0 0 0\n0 2 0\n0 0 2\n3 2 1 0\n", 0)
    assert np.array_equal(v, [[0, 0, 0], [0, 2, 0], [0, 0, 2]])
    assert np.array_equal(t, [[2, 1, 0]])


def test_parse_obj_corner_forms_negative_indices_polygons():
    text = ("# ShapeNet-style obj\n"
            "mtllib model.mtl\n"
            "v 0 0 0\nv 1 0 0\nv 1 1 0\n"
            "vn 0 0 1\nvt 0.5 0.5\n"
            "v 0 1 0   # trailing comment\n"
            "g part\n"
            "f 1 2 3\n"
            "f 1/1 3/1 4/1\n"
            "f 1//1 2//1 4//1\n"
            "f 1/1/1 2/1/1 3/1/1\n"
            "v 0.5 0.5 1\n"
            "f -1 -5 -4 -3 -2\n"                 # relative to the five vertices read so far: 5 1 2 3 4, a pentagon
            "usemtl red\n")
    v, t = m2p.parse_mesh(text, 1)
    assert np.array_equal(v, [[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0], [0.5, 0.5, 1]])
    assert np.array_equal(t, [[0, 1, 2], [0, 2, 3], [0, 1, 3], [0, 1, 2], [4, 0, 1], [4, 1, 2], [4, 2, 3]])


@pytest.mark.parametrize("text,fmt", [
    ("OFF\n3 1 0\n0 0 0\n1 0 0\n0 1 0\n3 0 1 3\n", 0),          # index == vertex count
    ("OFF\n3 1 0\n0 0 0\n1 0 0\n0 1 0\n3 0 -1 2\n", 0),         # negative index
    ("v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 4\n", 1),                # past the last vertex
    ("v 0 0 0\nv 1 0 0\nv 0 1 0\nf 0 1 2\n", 1),                # OBJ has no index 0
    ("v 0 0 0\nv 1 0 0\nf -1 -2 -3\nv 0 1 0\n", 1),             # relative index before the vertex exists
])
def test_parse_rejects_bad_indices(text, fmt):
    with pytest.raises(ValueError, match="index"):
        m2p.parse_mesh(text, fmt)


def test_parse_rejects_malformed_text():
    with pytest.raises(ValueError):
        m2p.parse_mesh("PLY\n3 1 0\n", 0)
    with pytest.raises(ValueError):
        m2p.parse_mesh("OFF\n3 1 0\n0 0 0\n1 0\n", 0)


def test_read_triangle_mesh_files(tmp_path):
    v, t = ref.box()
    off = tmp_path / "box.off"
    off.write_text("OFF\n%d %d 0\n" % (len(v), len(t)) + "".join("%r %r %r\n" % tuple(p) for p in v.tolist())
                   + "".join("3 %d %d %d\n" % tuple(f) for f in t.tolist()))
    obj = tmp_path / "box.obj"
    obj.write_text("".join("v %r %r %r\n" % tuple(p) for p in v.tolist()) + "".join("f %d %d %d\n" % tuple(f) for f in (t + 1).tolist()))
    for path in (off, obj):
        gv, gt = m2p.read_triangle_mesh(str(path))
        assert np.array_equal(gv, v) and np.array_equal(gt, t)
    with pytest.raises(ValueError):
        m2p.read_triangle_mesh(str(tmp_path / "box.stl"))


@pytest.mark.parametrize("mesh", ["icosphere", "box", "torus", "quad_soup"])
def test_area_cdf_is_cumsum_bit_for_bit(mesh):
    v, t = getattr(ref, mesh)()
    got = m2p.triangle_area_cdf(v, t)
    want = ref.area_cdf(v, t)
    assert got.dtype == np.float64 and np.array_equal(got.view(np.int64), want.view(np.int64))
    rng = np.random.default_rng(1)
    v2 = rng.standard_normal((5000, 3)) * 1e3
    t2 = rng.integers(0, 5000, (20000, 3)).astype(np.int32)
    assert np.array_equal(m2p.triangle_area_cdf(v2, t2).view(np.int64), ref.area_cdf(v2, t2).view(np.int64))


def test_area_cdf_rejects_flat_and_bad_meshes():
    v = np.array([[0, 0, 0], [1, 1, 1], [2, 2, 2]], np.float64)
    with pytest.raises(ValueError, match="no area"):
        m2p.triangle_area_cdf(v, np.array([[0, 1, 2], [0, 0, 1]], np.int32))
    with pytest.raises(ValueError, match="outside"):
        m2p.triangle_area_cdf(v, np.array([[0, 1, 3]], np.int32))


def test_get_rotate_matrix_orthonormal_and_reproducible():
    seen = set()
    for seed in range(16):
        m = m2p.get_rotate_matrix(seed)
        assert m.shape == (3, 3) and m.dtype == np.float64
        assert np.allclose(m @ m.T, np.eye(3), atol=1e-12)
        assert abs(abs(np.linalg.det(m)) - 1) < 1e-12
        assert np.array_equal(m, m2p.get_rotate_matrix(np.random.default_rng(seed)))
        seen.add(round(float(np.linalg.det(m))))
    assert seen == {-1, 1}                                   # the m[0,0] flip makes both handednesses


def test_offset_table_rule():
    t = ref.offset_table(10)
    assert len(t) == 4169 and np.array_equal(t[0], [0, 0, 0])
    d2 = (t * t).sum(1)
    assert (np.diff(d2) >= 0).all() and d2.max() == 100
    assert np.array_equal(t[1:7], [[-1, 0, 0], [0, -1, 0], [0, 0, -1], [0, 0, 1], [0, 1, 0], [1, 0, 0]])


def test_write_ply_normals_round_trip(tmp_path):
    rng = np.random.default_rng(3)
    pts = rng.integers(0, 256, (500, 3)).astype(np.int32)
    nrm = rng.standard_normal((500, 3)).astype(np.float32)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    nrm[0] = (-0.0, 1e-7, -3e-5)
    path = tmp_path / "c.ply"
    iop.write_ply_normals(str(path), pts, nrm)
    lines = path.read_text().split("\n")
    assert lines[:10] == ["ply", "format ascii 1.0", "element vertex 500", "property float x", "property float y", "property float z",
                          "property float nx", "property float ny", "property float nz", "end_header"]
    # the reference writer's text: str(int) and str(round(np.float64, 6)) per value
    for k in (0, 1, 250, 499):
        p, n = pts[k].astype("int"), nrm[k].astype("float")
        assert lines[10 + k] == " ".join([str(p[0]), str(p[1]), str(p[2]), str(round(n[0], 6)), str(round(n[1], 6)), str(round(n[2], 6))])
    assert lines[10] == "%d %d %d -0.0 0.0 -3e-05" % tuple(pts[0])
    got_p, got_n = iop.load_ply_normals(str(path))
    assert np.array_equal(got_p, pts) and np.allclose(got_n, nrm, atol=6e-7)
    assert np.array_equal(iop.load_ply_data(str(path)), pts)
