"""`--pointnums d2` on the host: the numpy definition (tests/_pointnums_d2_ref.py), fast form against from-scratch form on
engineered cubes, the normal quantiser, the chunk bound, the flags."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _pointnums_d2_ref as ref2                              # noqa: E402
import _pointnums_ref as ref                                  # noqa: E402

from pcgcv1_amd import pointnums as pn                        # noqa: E402


def _idx(cs, *xyz):
    return [(a * cs + b) * cs + c for a, b, c in xyz]


def _cube(cs, occupied, normals, high, rng, n=None, low_ties=False):
    """x with `occupied` voxels (xyz), their float normals by ascending voxel index, logits: `high` = [(xyz, logit)] on
    top of distinct (or, low_ties, repeated) values below -1"""
    vox = cs ** 3
    x = np.zeros(vox, np.float32)
    x[_idx(cs, *occupied)] = 1
    l = (-1.5 - rng.random(vox)).astype(np.float32)
    if low_ties:
        l = np.round(l * 8) / 8
    for xyz, val in high:
        l[_idx(cs, xyz)[0]] = val
    order = np.argsort(_idx(cs, *occupied))
    nrm = np.asarray(normals, np.float32).reshape(-1, 3)[order]
    return x.reshape(cs, cs, cs), l.reshape(cs, cs, cs), len(occupied) if n is None else n, nrm


def engineered_cubes_d2(cs=8, seed=11):
    """[(name, x [cs,cs,cs], logits, n, float normals [N,3] of the occupied voxels in ascending voxel index)]"""
    rng = np.random.default_rng(seed)
    vox = cs ** 3
    out = []
    # logit ties and signed zeros, random normals
    x = (rng.random(vox) < 0.08).astype(np.float32)
    z = rng.choice(np.array([-0.0, 0.0, 1.0, -1.0, 0.5], np.float32), vox)
    out.append(("signed_zero_ties", x.reshape(cs, cs, cs), z.reshape(cs, cs, cs), int(x.sum()),
                rng.standard_normal((int(x.sum()), 3)).astype(np.float32)))
    # B side: v = (3,3,3) is at distance 1 from (3,2,3) [normal x: plane error 0] and from (3,4,3) [normal y: error 1]; the
    # smaller voxel index (3,2,3) wins.  A side: p = (3,2,3) sees (4,2,3) [error 1] and (3,1,3) [error 0] at distance 1; the
    # lower rank wins, once each way.
    occ = [(3, 2, 3), (3, 4, 3), (6, 6, 6)]
    nrm = [(1, 0, 0), (0, 1, 0), (0, 0, 1)]
    out.append(("dist_ties_a", ) + _cube(cs, occ, nrm, [((3, 3, 3), 5.0), ((4, 2, 3), 4.0), ((3, 1, 3), 3.0), ((6, 6, 5), 2.0)], rng))
    out.append(("dist_ties_b", ) + _cube(cs, occ, nrm, [((3, 3, 3), 2.0), ((4, 2, 3), 3.0), ((3, 1, 3), 4.0), ((6, 6, 5), 2.0)], rng))
    # the same with the two B-side candidates' normals swapped: the tie-break now yields the larger error
    out.append(("dist_ties_c", ) + _cube(cs, occ, [(0, 1, 0), (1, 0, 0), (0, 0, 1)],
                                       [((3, 3, 3), 5.0), ((2, 2, 3), 4.0), ((3, 2, 4), 4.0), ((6, 6, 5), 2.0)], rng))
    # zero and non-finite normals
    occ = [(1, 1, 1), (2, 5, 3), (5, 2, 6), (6, 6, 1)]
    out.append(("zero_normal", ) + _cube(cs, occ, [(0, 0, 0), (np.nan, 1, 0), (np.inf, 0, 0), (0.3, -0.4, 1.2)],
                                       [((1, 2, 1), 3.0), ((2, 5, 5), 2.5), ((5, 3, 6), 2.0), ((6, 5, 1), 1.0)], rng, low_ties=True))
    # no occupied voxel
    out.append(("empty_p", ) + _cube(cs, [], np.zeros((0, 3)), [((1, 2, 3), 1.0)], rng, n=5))
    # p = (2,2,2), normal x: first (2,5,2) at distance 9, plane error 0; then (4,2,2) at distance 4, plane error 4: A2 rises
    out.append(("rise", ) + _cube(cs, [(2, 2, 2)], [(1, 0, 0)], [((2, 5, 2), 9.0), ((4, 2, 2), 8.0), ((2, 2, 3), 7.0), ((2, 2, 2), 6.0)], rng,
                                n=4))
    # a denser random cube with repeated logits
    x = (rng.random(vox) < 0.15).astype(np.float32)
    out.append(("random", x.reshape(cs, cs, cs), (np.round(rng.standard_normal(vox) * 2) / 2).astype(np.float32).reshape(cs, cs, cs),
                int(x.sum()), rng.standard_normal((int(x.sum()), 3)).astype(np.float32)))
    return out


def tiled_cubes_d2(cs=16, seed=12, count=3):
    """random 16^3 cubes whose occupied voxels and segment both exceed one 256-element tile; repeated and distinct logits"""
    rng = np.random.default_rng(seed)
    vox = cs ** 3
    out = []
    for i in range(count):
        x = (rng.random(vox) < 0.08 + 0.02 * i).astype(np.float32)
        l = rng.standard_normal(vox).astype(np.float32)
        if i % 2 == 0:
            l = (np.round(l * 4) / 4).astype(np.float32)
        n = int(x.sum())
        assert n > 256
        out.append(("tiled%d" % i, x.reshape(cs, cs, cs), l.reshape(cs, cs, cs), n, rng.standard_normal((n, 3)).astype(np.float32)))
    return out


CASES = engineered_cubes_d2()


@pytest.mark.parametrize("case", range(len(CASES)), ids=[c[0] for c in CASES])
def test_fast_form_equals_direct_masks(case):
    name, x, l, n, nrm = CASES[case]
    nq = ref2.quantise_normals(nrm)
    m, A2, B2 = ref2.curves_d2_ref(x, l, n, nq)
    K = int(pn.candidate_counts([n], x.size)[0])
    assert len(m) == len(A2) == len(B2) == K
    direct = ref2.curves_d2_direct(x, l, range(1, K + 1), nq)
    assert [tuple(int(v) for v in t) for t in zip(m, A2, B2)] == direct, name
    np.testing.assert_array_equal(m, ref.curves_ref(x, l, n)[0])            # the same sets as the D1 curves
    if name == "empty_p":
        assert not A2.any() and not B2.any()


def _case(name):
    return next(c for c in CASES if c[0] == name)


def test_tie_breaks_change_the_plane_error():
    """the engineered ties, worked by hand (unit: 1024^2 = one voxel^2 along a unit normal)"""
    one = 1024 ** 2
    _, x, l, n, nrm = _case("dist_ties_a")                     # ranks: (3,3,3), (4,2,3), (3,1,3), (6,6,5)
    m, A2, B2 = ref2.curves_d2_ref(x, l, n, ref2.quantise_normals(nrm))
    assert list(m[:3]) == [1, 2, 3]
    # k = 1: p1 = (3,2,3) lies in its plane (0), p2 = (3,4,3) is 1 off, p3 = (6,6,6) is 3 off; (3,3,3) ties between p1 and p2,
    # the smaller voxel index p1 wins and its normal sees no offset
    assert (A2[0], B2[0]) == (10 * one, 0)
    # k = 2: (4,2,3) ties with (3,3,3) for p1 at distance 1; the lower rank stays (the later one would add 1)
    assert (A2[1], B2[1]) == (10 * one, one)
    assert (A2[2], B2[2]) == (10 * one, one)
    _, x, l, n, nrm = _case("dist_ties_b")                     # ranks: (3,1,3), (4,2,3), then (3,3,3) and (6,6,5) tied
    m, A2, B2 = ref2.curves_d2_ref(x, l, n, ref2.quantise_normals(nrm))
    assert list(m[:3]) == [1, 2, 4]
    assert A2[0] == 18 * one                                   # 0 + 3^2 + 3^2
    assert A2[1] == 13 * one                                   # p1 keeps (3,1,3) on the tie (0); p2 and p3 move: 2^2 + 3^2
    _, x, l, n, nrm = _case("dist_ties_c")                     # the normals of p1 and p2 swapped
    _, _, B2 = ref2.curves_d2_ref(x, l, n, ref2.quantise_normals(nrm))
    assert B2[0] == one                                        # the same winner p1 now costs one voxel


def test_plane_error_can_rise():
    _, x, l, n, nrm = _case("rise")
    m, A2, B2 = ref2.curves_d2_ref(x, l, n, ref2.quantise_normals(nrm))
    assert list(A2[:4]) == [0, 4 * 1024 ** 2, 0, 0]      # far voxel in the plane, nearer voxel off it, then (2,2,3), then p itself
    assert list(m[:4]) == [1, 2, 3, 4]


def test_normal_quantisation():
    q = ref2.quantise_normals([[3, 4, 0], [0, 0, -2], [0, 0, 0], [np.nan, 1, 0], [np.inf, 0, 0], [1e-30, 0, 0], [1, 1, 1]])
    assert q.dtype == np.int32
    assert q.tolist() == [[614, 819, 0], [0, 0, -1024], [0, 0, 0], [0, 0, 0], [0, 0, 0], [1024, 0, 0], [591, 591, 591]]
    # half to even is the rounding in use: the quantiser is np.rint of the float64 quotient
    assert np.rint(np.array([0.5, 1.5, 2.5, -0.5, -1.5, 613.5, 614.5])).tolist() == [0, 2, 2, -0, -2, 614, 614]
    rng = np.random.default_rng(3)
    n = rng.standard_normal((2000, 3)).astype(np.float32)
    n64 = n.astype(np.float64)
    t = 1024.0 * n64 / np.sqrt(n64[:, 0] * n64[:, 0] + n64[:, 1] * n64[:, 1] + n64[:, 2] * n64[:, 2])[:, None]
    want = np.array([[round(float(v)) for v in row] for row in t])           # Python's round: half to even
    np.testing.assert_array_equal(ref2.quantise_normals(n), want)
    assert (np.abs(ref2.quantise_normals(n)).max() <= 1024) and ((ref2.quantise_normals(n).astype(np.int64) ** 2).sum(1) <= 1026 ** 2).all()


def test_voxel_normals_ref_lowest_index_wins():
    keys = np.array([7, -1, 3, 7, 3, 9], np.int64)
    nrm = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1], [0, 1, 0], [1, 0, 0], [0, -1, 0]], np.float32)
    uniq, q = ref2.voxel_normals_ref(keys, nrm)
    assert uniq.tolist() == [3, 7, 9]
    assert q.tolist() == [[0, 0, 1024], [1024, 0, 0], [0, -1024, 0]]


def test_point_keys_follow_preprocess():
    pts = np.array([[0, 0, 0], [63, 64, 5], [64, 0, 0], [1, 1, 1], [130, 3, 3], [63, 64, 5]], np.int32)
    pos = np.array([[1, 0, 0], [0, 0, 0], [0, 1, 0]])                       # first-appearance order; stored order sorts by key
    keys = pn.point_keys(pts, pos, 1.0, 64)
    vox = 64 ** 3
    # stored order (ordered_positions): (0,0,0), (1,0,0), (0,1,0)
    assert keys.tolist() == [0, 2 * vox + (63 * 64 + 0) * 64 + 5, 1 * vox, (64 + 1) * 64 + 1, -1, 2 * vox + (63 * 64 + 0) * 64 + 5]
    half = pn.point_keys(np.array([[1, 1, 1], [3, 3, 3], [5, 2, 0], [129, 0, 0]], np.int32), np.array([[0, 0, 0], [1, 0, 0]]), 0.5, 64)
    # round half to even in float32: 0.5 -> 0, 1.5 -> 2, 2.5 -> 2, 1 -> 1, 64.5 -> 64
    assert half.tolist() == [0, (2 * 64 + 2) * 64 + 2, (2 * 64 + 1) * 64, vox]


def test_chunk_plan_respects_the_bound():
    assert pn.plane_term_bound(64) == 3 * 63 * 63 * 1026 * 1026
    n_seg = [10, 20, 30, 5, 100, 7]
    n_pts = [3, 3, 3, 3, 3, 3]
    # the d1 plan: segment voxels only
    assert pn.chunk_plan(n_seg, chunk_seg=60) == [(0, 3), (3, 4), (4, 5), (5, 6)]
    assert pn.chunk_plan(n_seg, chunk_seg=1 << 23) == [(0, 6)]
    # with a term bound: (points + segment voxels) * bound < limit in every chunk that holds more than one cube
    bound = pn.plane_term_bound(64)
    for limit in (40 * bound, 41 * bound, 41 * bound + 1, 120 * bound, 1 << 62):
        plan = pn.chunk_plan(n_seg, n_pts, 1 << 23, bound, limit)
        assert [lo for lo, _ in plan] == [0] + [hi for _, hi in plan[:-1]] and plan[-1][1] == len(n_seg)
        for lo, hi in plan:
            el = sum(n_seg[lo:hi]) + sum(n_pts[lo:hi])
            assert el * bound < limit or hi - lo == 1
    assert pn.chunk_plan(n_seg, n_pts, 1 << 23, bound, 36 * bound + 1) == [(0, 2), (2, 3), (3, 4), (4, 5), (5, 6)]
    # greedy: never cuts earlier than it must
    assert pn.chunk_plan(n_seg, n_pts, 1 << 23, bound, 1 << 62) == [(0, 6)]
    # the worst cube the kernels take (256^3, every voxel occupied and selected) cannot wrap an int64 on either side
    assert 256 ** 3 * pn.plane_term_bound(256) < 1 << 62


def test_ladder_is_evals():
    from pcgcv1_amd import eval as rd
    assert pn.RHOS_D2 == rd.RHOS_D2 and 1.0 in pn.RHOS_D2
    assert pn.RHOS_D1 == rd.RHOS_D1


def test_guarantees_on_engineered_cubes():
    """the selection over the d2 curves of all engineered cubes: F2(chosen) <= F2(count) and every ladder entry"""
    curves = [ref2.curves_d2_ref(x, l, n, ref2.quantise_normals(nrm)) for _, x, l, n, nrm in CASES]
    nums = np.array([c[3] for c in CASES])
    K = np.array([len(c[0]) for c in curves])
    lad = pn.ladder_counts(nums, K, pn.RHOS_D2)
    ks, sums = ref.sweep_ref(curves, 64, lad)
    sum_n = int(sum(int(c[1].sum()) for c in CASES))
    sweep_sums = [tuple(int(v) for v in s) for s in sums[:65]]
    ladder_sums = [tuple(int(v) for v in s) for s in sums[65:]]
    kind, i, f = pn.select_assignment(sweep_sums, ladder_sums, pn.RHOS_D2, sum_n)
    for s in ladder_sums + sweep_sums:
        assert f <= pn.cloud_f(s[0], sum_n, s[1], s[2])


def test_flags(tmp_path, capsys):
    from pcgcv1_amd import test as cli
    from pcgcv1_amd.dataprocess import inout_points as iop
    pts = np.array([[1, 2, 3], [4, 5, 6]], np.int32)
    with_n, bare = str(tmp_path / "n.ply"), str(tmp_path / "bare.ply")
    iop.write_ply_normals(with_n, pts, np.array([[0, 0, 1], [1, 0, 0]], np.float32))
    iop.write_ply_data(bare, pts)
    a = cli.parse_args(["compress", with_n, "--pointnums", "d2"])                  # the ply's own normals
    assert a.pointnums == "d2" and a.estimate_normals is False
    a = cli.parse_args(["compress", bare, "--pointnums", "d2", "--estimate_normals"])
    assert a.pointnums == "d2" and a.estimate_normals is True
    assert cli.parse_args(["compress", bare]).pointnums == "count"
    assert cli.parse_args(["decompress", "compressed/x", "--pointnums", "d2"]).pointnums == "d2"     # ignored by decompress, as d1 is
    capsys.readouterr()
    for ply in (bare, str(tmp_path / "missing.ply")):                                # neither way: refused, both ways named
        with pytest.raises(SystemExit) as e:
            cli.parse_args(["compress", ply, "--pointnums", "d2"])
        assert e.value.code != 0
        err = capsys.readouterr().err
        assert "--estimate_normals" in err and "nx ny nz" in err
    with pytest.raises(SystemExit):
        cli.parse_args(["compress", with_n, "--pointnums", "d3"])
    with pytest.raises(SystemExit, match="pointnums"):
        cli.main(["compress", with_n, "--gpu", "2", "--pointnums", "d2"])
    with pytest.raises(SystemExit, match="estimate_normals"):
        cli.main(["compress", bare, "--estimate_normals"])


def test_optimizer_arguments():
    with pytest.raises(ValueError, match="metric"):
        pn.optimize_points_numbers(None, None, None, metric="d3")
    with pytest.raises(ValueError, match="voxel_normals"):
        pn.optimize_points_numbers(None, None, None, metric="d2")
