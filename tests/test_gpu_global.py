"""Global alignment on the device (csrc/global.hip: pcgc_feature_*, pcgc_ransac_score; pcgcv1_amd/register.py) against the rule in
numpy (tests/_global_ref.py): every stage is fed the reference's input to that stage and must give its output exactly, then
global_align on the five-sphere fixture follows the reference draw by draw, icp takes over from its pose, and the command line
does it all from two plies."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _global_ref as ref                                                # noqa: E402
import _register_ref as rref                                             # noqa: E402
from pcgcv1_amd import _lib, ingest, register                            # noqa: E402

_CACHE = {}
# the largest distance of a fixture source point from its true place where the reference loop ends, started from the reference's
# global pose; the device loop differs in summation order only: 10 % on top
REFERENCE_ICP_ERROR = 0.0200


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    _lib.require_gpu()


def _fixture():
    """the fixture and the reference's run on it, every stage kept; once"""
    if "fx" not in _CACHE:
        fx = ref.fixture()
        _CACHE["fx"] = (fx, ref.fixture_align(fx))
    return _CACHE["fx"]


def _random_cloud(n, seed, side=None, zero_normals=True):
    """n keypoints in a box with about 20 of them within 3, unit normals of either sign, a few of them zero"""
    rng = np.random.default_rng(seed)
    side = max(3.0, (n * 113.0 / 20.0) ** (1.0 / 3.0)) if side is None else side
    kp = rng.uniform(0.0, side, (n, 3)).astype(np.float32)
    nrm = rng.normal(size=(n, 3))
    nrm = ref.unit_normals(nrm)
    if zero_normals and n > 10:
        nrm[rng.choice(n, n // 10, replace=False)] = 0.0
    return kp, nrm


def _check_stages(kp, nrm, r, what, cells=None):
    """stage 1 against the reference; stage 2, fed the reference's S and k, against the reference"""
    S, k = register.feature_pairs(kp, nrm, r, cells)
    want_S, want_k = ref.pairs(kp, nrm, r)
    assert S.dtype == np.uint32 and k.dtype == np.int32 and S.shape == (len(kp), 33)
    assert np.array_equal(k, want_k), (what, np.nonzero(k != want_k)[0][:5].tolist())
    assert np.array_equal(S, want_S), (what, np.nonzero((S != want_S).any(1))[0][:5].tolist())
    assert np.array_equal(S.reshape(len(kp), 3, 11).sum(2), np.repeat(want_k[:, None], 3, 1))
    feat, valid = register.feature_combine(kp, nrm, r, want_S, want_k, cells)
    want_feat, want_valid = ref.combine(kp, nrm, r, want_S, want_k)
    assert feat.dtype == np.uint8 and feat.shape == (len(kp), 36) and np.array_equal(valid, want_valid), what
    assert np.array_equal(feat, want_feat), (what, np.nonzero((feat != want_feat).any(1))[0][:5].tolist())
    assert not feat[:, 33:].any()
    return S, k, feat, valid


# ---------------------------------------------------------------------------- 1, 2: the descriptor
@pytest.mark.parametrize("n", (1, 2, 63, 65, 257))
def test_pairs_and_combine_sizes(n):
    kp, nrm = _random_cloud(n, 100 + n)
    S, k, feat, valid = _check_stages(kp, nrm, 3.0, "n = %d" % n)
    if n >= 63:
        assert k.max() > 5 and valid.sum() > n // 2 and (k == 0).any()
    else:
        _check_stages(np.array([[0, 0, 0], [1, 2, 2]], np.float32)[:n], np.array([[0, 0, 1], [0, 1, 0]], np.float32)[:n], 3.0, "near")


def test_pairs_and_combine_on_the_fixture():
    """the source keypoints of the fixture, 4 293 of them, radius 8: more than one workgroup pass, cells of edge 8"""
    _, out = _fixture()
    S, k, feat, valid = _check_stages(out["source_kp"], out["source_kp_normals"], ref.RADIUS, "fixture")
    assert np.array_equal(S, out["source_pairs"][0]) and np.array_equal(feat, out["source_feat"][0]) and k.max() > 150
    got = register.features(out["target_kp"], out["target_kp_normals"], ref.RADIUS)         # the two stages in one go
    assert np.array_equal(got[0], out["target_feat"][0]) and np.array_equal(got[1], out["target_feat"][1])


def test_pairs_edge_cases():
    """a neighbour at exactly r and one just beyond; two coincident points; a zero normal; a normal along u (f = 1, bin 10) and
    one across it (f = 0, bin 0)"""
    beyond = np.nextafter(np.float32(3.0), np.float32(4.0))
    kp = np.array([[0, 0, 0], [3, 0, 0], [0, beyond, 0], [0, 0, 2], [0, 0, 2], [1, 1, 0], [-2, 0, 0]], np.float32)
    nrm = np.array([[1, 0, 0], [0, 0, 1], [0, 1, 0], [1, 0, 0], [0, 0, -1], [0, 0, 0], [-1, 0, 0]], np.float32)
    S, k, feat, valid = _check_stages(kp, nrm, 3.0, "edge cases")
    # point 0: neighbours 1 (at exactly 3), 3 and 4 (coincident with each other, both count), 6; not 2 (beyond), not 5 (zero normal)
    assert k.tolist()[0] == 4 and k[5] == 0 and not S[5].any()
    assert k.tolist() == [4, 1, 0, 2, 2, 0, 3]                 # 3 and 4 do not see each other: d2 = 0
    assert S[0, 10] == 2 and S[0, 0] == 2                      # n_0 = x: along u for points 1 and 6, across it for 3 and 4
    assert S[0, 11 + 10] == 2                                  # f2 = 1: the normals of 6 (x) and 4 (z) lie along their u
    assert S[0, 22 + 10] == 2 and S[0, 22] == 2                # f3: |n_0 . n_j| = 1 for 3 and 6, 0 for 1 and 4
    assert not S[2].any() and not valid[2] and not valid[5] and valid[[0, 1, 3, 4, 6]].all()
    flipped = register.feature_pairs(kp, -nrm, 3.0)
    assert np.array_equal(flipped[0], S) and np.array_equal(flipped[1], k)                    # the sign of a normal does not matter
    mixed = register.feature_pairs(kp, nrm * np.array([[1], [-1], [1], [-1], [1], [1], [-1]], np.float32), 3.0)
    assert np.array_equal(mixed[0], S)


def test_cells_of_edge_two_with_a_negative_origin():
    kp, nrm = _random_cloud(300, 9)
    kp = (kp - np.float32(37.3)).astype(np.float32)
    lo, hi = np.floor(kp.astype(np.float64).min(0) / 2.0), np.floor(kp.astype(np.float64).max(0) / 2.0)
    cells = (2.0, int(lo[0]), int(lo[1]), int(lo[2]), int((hi - lo).max()) + 1)
    assert cells[1] < 0
    S, k, _, _ = _check_stages(kp, nrm, 3.0, "edge 2", cells)                                 # a window of two cells each way
    auto = register.feature_pairs(kp, nrm, 3.0)                                             # edge 4, one cell each way
    assert register.feature_cells(kp, 3.0)[0] == 4.0 and np.array_equal(auto[0], S) and np.array_equal(auto[1], k)


def test_combine_when_every_neighbour_has_no_neighbours():
    """S and k are taken as given: a keypoint with k = 5 whose neighbours all carry k = 0 has T = 25 and stays valid"""
    kp, nrm = _random_cloud(65, 3, zero_normals=False)
    S = np.zeros((65, 33), np.uint32)
    k = np.zeros(65, np.int32)
    k[7] = 5
    S[7, [0, 11, 22]] = (2, 5, 1)
    S[7, [3, 32]] = (3, 4)
    feat, valid = register.feature_combine(kp, nrm, 3.0, S, k)
    want_feat, want_valid = ref.combine(kp, nrm, 3.0, S, k)
    assert np.array_equal(feat, want_feat) and np.array_equal(valid, want_valid)
    assert valid[7] and valid.sum() == 1 + len(set(ref.neighbours(kp, nrm, 3.0)[0][ref.neighbours(kp, nrm, 3.0)[1] == 7].tolist()))
    assert feat[7, 0] == 102 and feat[7, 11] == 255 and feat[7, 3] == 153 and feat[7, 22] == 51 and feat[7, 32] == 204


# ---------------------------------------------------------------------------- 3: match
def _rows(n, seed, spread=256):
    rng = np.random.default_rng(seed)
    f = np.zeros((n, 36), np.uint8)
    f[:, :33] = rng.integers(0, spread, (n, 33))
    return f


@pytest.mark.parametrize("m", (1, 64, 1000))
@pytest.mark.parametrize("n", (1, 63, 257))
def test_match_sizes(n, m):
    """random rows, some invalid on either side, duplicated target rows (the lowest index wins), a tail tile that is not full"""
    rng = np.random.default_rng(n * 1000 + m)
    fs, ft = _rows(n, n), _rows(m, 7000 + m)
    vs, vt = rng.random(n) < 0.9, rng.random(m) < 0.8
    if m >= 64:
        ft[m - 1] = ft[m // 2] = ft[5]                           # three equal rows, one of them in the last tile
        vt[[5, m // 2, m - 1]] = (False, True, True)           # the first of them invalid: the second wins
        fs[0] = ft[5]
        vs[0] = True
        ft[9] = ft[8]
        vt[[8, 9]] = True
        fs[n - 1] = ft[9]
        vs[n - 1] = True
    j, dist = register.match_features(fs, vs, ft, vt)
    want_j, want_dist = ref.match(fs, vs, ft, vt)
    assert j.dtype == np.int32 and dist.dtype == np.uint32
    assert np.array_equal(j, want_j) and np.array_equal(dist, want_dist)
    assert np.array_equal(j < 0, ~vs | ~vt.any()) and np.all(dist[j < 0] == 0xFFFFFFFF)
    if m >= 64:
        assert j[n - 1] == 8 and dist[n - 1] == 0 and (n == 1 or (j[0] == m // 2 and dist[0] == 0))
    # brute force on one row, in integers
    i = int(np.argmax(vs))
    if vt.any():
        d = ((fs[i, :33].astype(np.int64) - ft[:, :33].astype(np.int64)) ** 2).sum(1)
        d[~vt] = 2 ** 40
        assert j[i] == int(np.argmin(d)) and dist[i] == d.min()


def test_match_extremes():
    """the largest distance 33 * 255^2 fits; the bytes behind the bins are not data; no valid target row"""
    fs, ft = np.zeros((3, 36), np.uint8), np.zeros((300, 36), np.uint8)
    ft[:, :33] = 255
    j, dist = register.match_features(fs, np.ones(3, bool), ft, np.ones(300, bool))
    assert j.tolist() == [0, 0, 0] and dist.tolist() == [33 * 255 * 255] * 3
    a, b = _rows(63, 1, 8), _rows(1000, 2, 8)                    # few levels: many ties
    plain = register.match_features(a, np.ones(63, bool), b, np.ones(1000, bool))
    want = ref.match(a, np.ones(63, bool), b, np.ones(1000, bool))
    assert np.array_equal(plain[0], want[0]) and np.array_equal(plain[1], want[1])
    a[:, 33:], b[:, 33:] = 77, 200
    padded = register.match_features(a, np.ones(63, bool), b, np.ones(1000, bool))
    assert np.array_equal(padded[0], plain[0]) and np.array_equal(padded[1], plain[1])
    none = register.match_features(a, np.ones(63, bool), b, np.zeros(1000, bool))
    assert np.all(none[0] == -1) and np.all(none[1] == 0xFFFFFFFF)


# ---------------------------------------------------------------------------- 4: score
def _poses(K, seed):
    """rotations and shifts about a cloud in [0, 40]^3 whose entries are no float32 numbers; one in three close to the identity"""
    rng = np.random.default_rng(seed)
    out = np.empty((K, 12))
    for k in range(K):
        R = rref.rodrigues(rng.normal(size=3) * (0.02 if k % 3 == 0 else 1.0))
        c = np.full(3, 20.0)
        out[k] = np.concatenate([R.reshape(9), c - R @ c + rng.normal(size=3) * (0.5 if k % 3 == 0 else 5.0)])
    return out


def _score_case(C):
    if ("score", C) not in _CACHE:
        rng = np.random.default_rng(C)
        P = rng.uniform(0.0, 40.0, (C, 3)).astype(np.float32)
        Q = (P + rng.normal(size=(C, 3)) * 1.0).astype(np.float32)
        poses = _poses(5000, 11)
        assert not np.array_equal(poses, poses.astype(np.float32).astype(np.float64))
        _CACHE[("score", C)] = (P, Q, poses, ref.score(poses, P, Q, 2.0))      # the reference once for all K
    return _CACHE[("score", C)]


@pytest.mark.parametrize("C", (1, 100, 2000))
@pytest.mark.parametrize("K", (1, 63, 257, 5000))
def test_score_sizes(K, C):
    P, Q, poses, want = _score_case(C)
    got = register.score_poses(poses[:K], P, Q, 2.0)
    assert got.dtype == np.int32 and np.array_equal(got, want[:K])
    if C == 2000 and K == 5000:
        assert got.max() > 1000 and got.min() < 50


def test_score_at_exactly_the_distance_and_with_a_bad_pose():
    P = np.array([[0, 0, 0], [1, 1, 1], [2, 0, 0]], np.float32)
    Q = np.array([[3, 4, 0], [1, 1, 1], [2, 0, 12]], np.float32)
    eye = np.concatenate([np.eye(3).reshape(9), np.zeros(3)])
    below = float(np.nextafter(5.0, 0.0))
    assert register.score_poses(eye, P, Q, 5.0).tolist() == [2] and register.score_poses(eye, P, Q, below).tolist() == [1]
    assert register.score_poses(eye, P, Q, 12.0).tolist() == [3]
    bad = np.stack([eye, eye, eye])
    bad[1, 4] = np.nan
    bad[2, 9] = np.inf
    assert register.score_poses(bad, P, Q, 5.0).tolist() == [2, 0, 0] == ref.score(bad, P, Q, 5.0).tolist()
    # the float32 rounding of the moved point is part of the rule
    shift = eye.copy()
    shift[9] = 1e-9
    P1, Q1 = np.array([[1.0, 0, 0]], np.float32), np.array([[3.0, 0, 0]], np.float32)
    assert register.score_poses(shift, P1, Q1, 2.0).tolist() == [1] == ref.score(shift, P1, Q1, 2.0).tolist()


# ---------------------------------------------------------------------------- determinism, robustness
def test_two_runs_give_the_same_bytes():
    kp, nrm = _random_cloud(257, 5)
    first = register.feature_pairs(kp, nrm, 3.0)
    again = register.feature_pairs(kp, nrm, 3.0)
    assert first[0].tobytes() == again[0].tobytes() and first[1].tobytes() == again[1].tobytes()
    f1, f2 = register.features(kp, nrm, 3.0), register.features(kp, nrm, 3.0)
    assert f1[0].tobytes() == f2[0].tobytes() and f1[1].tobytes() == f2[1].tobytes()
    a, b = _rows(257, 1, 6), _rows(1000, 2, 6)
    m1, m2 = (register.match_features(a, np.ones(257, bool), b, np.ones(1000, bool)) for _ in range(2))
    assert m1[0].tobytes() == m2[0].tobytes() and m1[1].tobytes() == m2[1].tobytes()
    P, Q, poses, _ = _score_case(2000)
    assert register.score_poses(poses[:257], P, Q, 2.0).tobytes() == register.score_poses(poses[:257], P, Q, 2.0).tobytes()


def test_bad_arguments_are_refused():
    import torch
    lib = _lib.hip()
    kp, nrm = _random_cloud(63, 2)
    c = register._FeatureCloud(kp, nrm, 3.0)
    S = torch.zeros((63, 33), dtype=torch.int32, device=c.dev)
    k = torch.zeros(63, dtype=torch.int32, device=c.dev)
    feat = torch.zeros((63, 36), dtype=torch.uint8, device=c.dev)
    valid = torch.zeros(63, dtype=torch.uint8, device=c.dev)
    h, ox, oy, oz, res = c.cells

    def pairs(kp_d=c.kp, n=63, h=h, res=res, radius=3.0, ws_bytes=c.ws.numel(), S=S):
        return lib.pcgc_feature_pairs(_lib.dptr(kp_d), _lib.dptr(c.normals), n, h, ox, oy, oz, res, radius, _lib.dptr(S), _lib.dptr(k),
                                      _lib.dptr(c.ws), ws_bytes, _lib.stream())

    def combine(radius=3.0, feat=feat, ws_bytes=c.ws.numel(), n=63):
        return lib.pcgc_feature_combine(_lib.dptr(c.kp), _lib.dptr(c.normals), n, h, ox, oy, oz, res, radius, _lib.dptr(S), _lib.dptr(k),
                                        _lib.dptr(feat), _lib.dptr(valid), _lib.dptr(c.ws), ws_bytes, _lib.stream())
    assert pairs() == 0 and combine() == 0
    for bad in (dict(kp_d=None), dict(n=0), dict(n=-1), dict(n=(1 << 24) + 1), dict(h=3.0), dict(h=0.5), dict(res=0), dict(res=1025),
                dict(radius=0.0), dict(radius=-1.0), dict(radius=float("nan")), dict(radius=float("inf")), dict(radius=4.0 * h),
                dict(ws_bytes=c.ws.numel() - 1), dict(S=None)):
        assert pairs(**bad) != 0, bad
    assert "pcgc_feature_pairs" in lib.pcgc_last_error().decode()
    assert pairs(radius=float(np.nextafter(4.0 * h, 0.0))) == 0                              # the widest window there is
    for bad in (dict(radius=4.0 * h), dict(radius=float("nan")), dict(feat=None), dict(ws_bytes=0), dict(n=0)):
        assert combine(**bad) != 0, bad
    assert lib.pcgc_feature_workspace_bytes(0, 10) == 0 and lib.pcgc_feature_workspace_bytes(8, 0) == 0
    assert lib.pcgc_feature_workspace_bytes(8, (1 << 24) + 1) == 0 and lib.pcgc_feature_workspace_bytes(8, 63) == c.ws.numel()
    assert lib.pcgc_feature_match_workspace_bytes(0) == 0 and lib.pcgc_feature_match_workspace_bytes(63) == 512
    rows = torch.zeros((64, 36), dtype=torch.uint8, device=c.dev)
    flags = torch.ones(64, dtype=torch.uint8, device=c.dev)
    j = torch.zeros(64, dtype=torch.int32, device=c.dev)
    ws = torch.zeros(512, dtype=torch.uint8, device=c.dev)

    def match(fs=rows, n=64, m=64, ws_bytes=512, j=j, offset=0):
        ptr = None if fs is None else _lib.dptr(fs).value + offset
        return lib.pcgc_feature_match(ptr, _lib.dptr(flags), n, _lib.dptr(rows), _lib.dptr(flags), m, _lib.dptr(j), _lib.dptr(k),
                                      _lib.dptr(ws), ws_bytes, _lib.stream())
    assert match() == 0
    for bad in (dict(fs=None), dict(n=0), dict(m=0), dict(ws_bytes=511), dict(j=None), dict(offset=1, n=63)):
        assert match(**bad) != 0, bad
    poses = torch.zeros((4, 12), dtype=torch.float64, device=c.dev)

    def score(poses=poses, K=4, C=21, dist=2.0):
        return lib.pcgc_ransac_score(_lib.dptr(poses), K, _lib.dptr(c.kp), _lib.dptr(c.kp), C, dist, _lib.dptr(j), _lib.stream())
    assert score() == 0
    for bad in (dict(poses=None), dict(K=0), dict(C=0), dict(dist=0.0), dict(dist=float("nan")), dict(dist=float("inf"))):
        assert score(**bad) != 0, bad
    with pytest.raises(ValueError, match="normals for"):
        register.feature_pairs(kp, nrm[:10], 3.0)


def test_a_nan_keypoint_or_an_unsorted_cloud_raises_the_flag_and_the_next_call_works():
    kp, nrm = _random_cloud(257, 6)
    want = ref.pairs(kp, nrm, 3.0)
    bad = kp.copy()
    bad[100, 1] = np.nan
    with pytest.raises(RuntimeError, match="pcgc_feature_pairs"):
        register.feature_pairs(bad, nrm, 3.0)
    with pytest.raises(RuntimeError, match="pcgc_feature_combine"):
        register.feature_combine(bad, nrm, 3.0, want[0], want[1])
    c = register._FeatureCloud(kp, nrm, 3.0)
    good = c.pairs()
    sorted_kp = c.kp
    c.kp = sorted_kp.flip(0).contiguous()                       # descending cell keys
    with pytest.raises(RuntimeError, match="pcgc_feature_pairs"):
        c.pairs()
    c.kp = (sorted_kp + 4096.0).contiguous()                    # outside the cells
    with pytest.raises(RuntimeError, match="pcgc_feature_pairs"):
        c.pairs()
    c.kp = sorted_kp                                            # the same workspace again: the flag is each call's own
    S, k = c.pairs()
    assert np.array_equal(c.back(S).view(np.uint32), want[0]) and np.array_equal(c.back(k), want[1])
    assert np.array_equal(S.cpu().numpy(), good[0].cpu().numpy())
    # normals that are not numbers make a keypoint unusable, nothing more
    odd = nrm.copy()
    odd[3] = (np.nan, 0, 1)
    odd[4] = (np.inf, 0, 0)
    S2, k2 = register.feature_pairs(kp, odd, 3.0)
    w2 = ref.pairs(kp, odd, 3.0)
    assert np.array_equal(S2, w2[0]) and np.array_equal(k2, w2[1]) and k2[3] == 0 and k2[4] == 0


# ---------------------------------------------------------------------------- the whole of it
def _device_align():
    if "align" not in _CACHE:
        fx, _ = _fixture()
        _CACHE["align"] = register.global_align(fx["source"], fx["target"], fx["source_normals"], fx["target_normals"], ref.FEATURE_VOXEL,
                                                ref.RADIUS, ref.CORR_DIST, ref.MIN_EDGE, ref.DRAWS, ref.SEED, ref.MIN_INLIERS)
    return _CACHE["align"]


def test_global_align_follows_the_reference_on_the_fixture():
    fx, want = _fixture()
    ks, ns = register.keypoints(fx["source"], fx["source_normals"], ref.FEATURE_VOXEL)
    kt, nt = register.keypoints(fx["target"], fx["target_normals"], ref.FEATURE_VOXEL)
    assert ks.tobytes() == want["source_kp"].tobytes() and ns.tobytes() == want["source_kp_normals"].tobytes()
    assert kt.tobytes() == want["target_kp"].tobytes() and nt.tobytes() == want["target_kp_normals"].tobytes()
    P, Q, rows, cols = register.correspondences(ks, *register.features(ks, ns, ref.RADIUS), kt, *register.features(kt, nt, ref.RADIUS))
    assert np.array_equal(rows, want["rows"]) and np.array_equal(cols, want["cols"])              # the correspondences are identical
    assert P.tobytes() == want["P"].tobytes() and Q.tobytes() == want["Q"].tobytes()
    counts = register.score_poses(want["poses"], P, Q, ref.CORR_DIST)
    assert np.array_equal(counts, want["counts"])                                                # hypothesis by hypothesis
    got = _device_align()
    print("fixture on the device: %d correspondences, %d hypotheses, draw %d, %d inliers raw, %d refined, %.3f voxel from the truth" % (
        got["correspondences"], got["hypotheses"], got["draw"], got["raw_inliers"], got["inliers"], ref.point_error(got["R"], got["t"], fx)))
    for key in ("correspondences", "hypotheses", "draw", "draws", "raw_inliers", "inliers"):
        assert got[key] == want[key], key
    assert np.abs(got["R"] - want["R"]).max() <= 1e-12 and np.abs(got["t"] - want["t"]).max() <= 1e-12
    assert ref.point_error(got["R"], got["t"], fx) <= ref.CORR_DIST


def test_icp_takes_over_from_the_global_pose():
    """plane mode from the pose global_align found; every fourth source point, which the reference loop still walks in a few
    seconds.  The same steps, the same points inside the last gate, poses no further apart than tol: the existing loop test's
    terms.  The reference ends 0.0199 voxel from the truth at most (over all source points)."""
    fx, _ = _fixture()
    start = _device_align()
    src = fx["source"][::4]
    tn = register._unit_normals(fx["target_normals"], len(fx["target"]))
    want = rref.icp(src, fx["target"], tn, "plane", (4.0, 2.0, 1.0), 50, 1e-3, init=(start["R"], start["t"]))
    got = register.icp(src, fx["target"], fx["target_normals"], "plane", (4.0, 2.0, 1.0), 50, 1e-3, init=(start["R"], start["t"]))
    p = src.astype(np.float64)
    apart = float(np.linalg.norm((p @ got["R"].T + got["t"]) - (p @ want["R"].T + want["t"]), axis=1).max())
    err, err_ref = ref.point_error(got["R"], got["t"], fx), ref.point_error(want["R"], want["t"], fx)
    print("icp from the global pose: steps %s, n_used %d, device and reference %.3g voxel apart, largest point error %.5f (reference "
          "%.5f) voxel" % (got["iterations"], got["n_used"], apart, err, err_ref))
    assert got["iterations"] == want["iterations"] and got["converged"] and want["converged"]
    assert got["n_used"] == want["n_used"] and got["fitness"] == want["fitness"] and apart <= 1e-3
    assert abs(got["rmse"] - want["rmse"]) < 1e-6 and abs(got["plane_rmse"] - want["plane_rmse"]) < 1e-6
    assert err_ref <= REFERENCE_ICP_ERROR and err <= 1.1 * REFERENCE_ICP_ERROR


def _scans(fx):
    return [(fx["target"].astype(np.float64), None, fx["target_normals"]), (fx["source"].astype(np.float64), None, fx["source_normals"])]


def test_the_need_for_it_shown():
    """the fixture pair as two scans, voxels of edge 1: icp alone is lost, with global_init the source lands in its place"""
    fx, _ = _fixture()
    try:
        lost = register.register_scans(_scans(fx), voxel_size=1.0, metric="plane")["poses"][1]
        print("without global_init: steps %s, converged %s, fitness %.3f" % (lost["iterations"], lost["converged"], lost["fitness"]))
        assert lost["fitness"] < 0.3 and "global" not in lost
        assert ref.point_error(lost["R"], lost["t"], fx) > 10.0
    except ValueError as e:
        assert "nothing lies within max_dist" in str(e)
    options = dict(feature_voxel=ref.FEATURE_VOXEL, radius=ref.RADIUS, corr_dist=ref.CORR_DIST, min_edge=ref.MIN_EDGE, draws=ref.DRAWS,
                   seed=ref.SEED, min_inliers=ref.MIN_INLIERS)
    out = register.register_scans(_scans(fx), voxel_size=1.0, metric="plane", global_init=True, global_options=options)
    r = out["poses"][1]
    err = ref.point_error(r["R"], r["t"], fx)
    print("with global_init: %s, steps %s, converged %s, fitness %.3f, largest point error %.5f voxel" % (
        r["global"], r["iterations"], r["converged"], r["fitness"], err))
    assert sorted(r["global"]) == ["correspondences", "draw", "hypotheses", "inliers"] and r["global"]["inliers"] >= ref.MIN_INLIERS
    assert r["fitness"] > 0.7 and err <= 1.1 * REFERENCE_ICP_ERROR
    assert "global" not in out["poses"][0]


def test_scans_without_normals_get_them_estimated():
    """the same pair with no normals at all: the plane metric's are estimated on the target's voxels, and so are both clouds'
    for the descriptors.  The margin is thin with such normals (150 inliers against 135 for the best wrong pose in
    the numpy rule, the coarse pose 3.3 voxels off), and they set the accuracy icp reaches, 0.1 to 0.2 voxel in §7h: the pose
    must be within half a voxel, where icp alone ends 40 voxels off."""
    fx, _ = _fixture()
    scans = [(fx["target"].astype(np.float64), None, None), (fx["source"].astype(np.float64), None, None)]
    options = dict(feature_voxel=ref.FEATURE_VOXEL, radius=ref.RADIUS, corr_dist=ref.CORR_DIST, min_edge=ref.MIN_EDGE, draws=ref.DRAWS,
                   seed=ref.SEED, min_inliers=ref.MIN_INLIERS)
    r = register.register_scans(scans, voxel_size=1.0, metric="plane", estimate_normals=True, global_init=True,
                                global_options=options)["poses"][1]
    err = ref.point_error(r["R"], r["t"], fx)
    print("estimated normals: %s, steps %s, converged %s, fitness %.3f, largest point error %.4f voxel" % (
        r["global"], r["iterations"], r["converged"], r["fitness"], err))
    assert r["global"]["correspondences"] > 4000 and r["global"]["inliers"] >= 100 and r["fitness"] > 0.7 and err <= 0.5


UNIT = 0.01                  # scanner units per voxel of the fixture


def _write_scan(name, points, normals):
    """an ASCII ply of float positions with normals; repr holds a float64 as it is"""
    with open(name, "w") as f:
        f.write("ply\nformat ascii 1.0\nelement vertex %d\nproperty double x\nproperty double y\nproperty double z\n"
                "property float nx\nproperty float ny\nproperty float nz\nend_header\n" % len(points))
        for row in np.concatenate([points, normals.astype(np.float64)], 1).tolist():
            f.write(" ".join(repr(v) for v in row) + "\n")


def test_command_line_round_trip(tmp_path, capsys):
    """Two plies of the fixture in scanner units, normals of either sign in them.  poses.json carries the "global" block, and the
    merged ply is what ingest.voxelize_scan gives for the union under the reference's poses, but for the voxels a point within
    1e-3 voxel of a boundary touches (test_three_scans_merge_as_the_reference_poses_merge_them).  The coarse pose lies within
    corr_dist = 2, so the schedule starts at a gate of 2."""
    from pcgcv1_amd.dataprocess.inout_points import load_ply_scan
    fx, _ = _fixture()
    scans = [fx["target"].astype(np.float64) * UNIT, fx["source"].astype(np.float64) * UNIT]
    normals = [fx["target_normals"], fx["source_normals"]]
    names = [str(tmp_path / ("scan%d.ply" % k)) for k in range(2)]
    for name, p, n in zip(names, scans, normals):
        _write_scan(name, p, n)
        back = load_ply_scan(name)
        assert np.array_equal(back[0], p) and back[1] is None and np.array_equal(back[2], n)
    merged = str(tmp_path / "merged.ply")
    argv = ["--input"] + names + ["--output", merged, "--voxel_size", repr(UNIT), "--max_dist", "2,1", "--global_init",
                                  "--feature_voxel", repr(ref.FEATURE_VOXEL), "--seed", str(ref.SEED), "--attributes", "normals"]
    register.main(argv)
    printed = capsys.readouterr().out
    assert "global start from draw" in printed and "NOT converged" not in printed and "wrote " in printed
    poses = register.read_poses(register.poses_path(merged))
    assert "global" not in poses[0] and sorted(poses[1]["global"]) == ["correspondences", "draw", "hypotheses", "inliers"]
    # the reference's poses on the grid the command line registers on
    frame = ingest.fit_frame(scans[0], voxel_size=UNIT)
    src, tgt = register.to_grid(scans[1], frame), register.to_grid(scans[0], frame)
    coarse = ref.global_align(src, tgt, normals[1], normals[0], ref.FEATURE_VOXEL, ref.RADIUS, ref.CORR_DIST, ref.MIN_EDGE, ref.DRAWS,
                              ref.SEED, ref.MIN_INLIERS)
    assert poses[1]["global"] == {key: coarse[key] for key in ("inliers", "correspondences", "hypotheses", "draw")}
    r = rref.icp(src, tgt, register._unit_normals(normals[0], len(tgt)), "plane", (2.0, 1.0), 50, 1e-3, init=(coarse["R"], coarse["t"]))
    R, t = register.pose_to_scan_units(r["R"], r["t"], frame)
    moved = np.linalg.norm((scans[1] @ R.T + t) - (scans[1] @ poses[1]["pose"][:3, :3].T + poses[1]["pose"][:3, 3]), axis=1).max() / UNIT
    err = float(np.linalg.norm(scans[1] @ poses[1]["pose"][:3, :3].T + poses[1]["pose"][:3, 3] - fx["source_true"] * UNIT, axis=1).max()) / UNIT
    print("command line: %s, steps %s, device and reference %.3g voxel apart, largest point error %.4f voxel" % (
        poses[1]["global"], poses[1]["iterations"], moved, err))
    assert poses[1]["iterations"] == r["iterations"] and poses[1]["converged"] and moved <= 1e-3 and err <= 1.1 * REFERENCE_ICP_ERROR
    union = np.concatenate([scans[0], scans[1] @ R.T + t])
    w_points, _, _, w_counts, w_frame, _ = ingest.voxelize_scan(union, voxel_size=UNIT)
    points = load_ply_scan(merged)[0].astype(np.int32)
    out_frame = ingest.read_frame(ingest.frame_path(merged))
    assert out_frame == w_frame
    u = (union - out_frame.origin) / out_frame.step + 0.5
    near = np.abs(u - np.rint(u)).min(1) < 1e-3
    res = 1 << out_frame.bits

    def keys(v):
        v = np.clip(v, 0, out_frame.R).astype(np.int64)
        return (v[:, 0] * res + v[:, 1]) * res + v[:, 2]
    touched = np.unique(np.concatenate([keys(np.floor(u[near] + (np.array(d) - 1.0) * 1e-3)) for d in np.ndindex(3, 3, 3)]))
    k_got, k_want = keys(points), keys(w_points)
    keep_got, keep_want = ~np.isin(k_got, touched), ~np.isin(k_want, touched)
    assert keep_want.sum() > 0.97 * len(w_points)
    assert np.array_equal(points[keep_got], w_points[keep_want])
    # refused together with a start of the caller's
    with pytest.raises(SystemExit):
        register.main(argv + ["--init", register.poses_path(merged)])
