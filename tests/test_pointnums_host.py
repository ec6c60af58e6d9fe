"""Encoder-side point counts (pcgcv1_amd/pointnums.py) on the host: the numpy restatement against the decoder's own mask
rule, the selection's tie rules and guarantees, and the --pointnums flag."""
import os
import sys
from fractions import Fraction

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _pointnums_ref as ref                                  # noqa: E402

from pcgcv1_amd import pointnums as pn                        # noqa: E402


def engineered_cubes(cs=8, seed=5):
    """(name, x [cs,cs,cs], logits, n): ties, signed zeros, a constant cube, n = 1"""
    rng = np.random.default_rng(seed)
    vox = cs ** 3
    out = []
    x = (rng.random(vox) < 0.08).astype(np.float32)
    out.append(("repeated", x, np.round(rng.standard_normal(vox) * 2).astype(np.float32) / 2, int(x.sum())))
    z = rng.choice(np.array([-0.0, 0.0, 1.0, -1.0], np.float32), vox)
    x2 = (rng.random(vox) < 0.05).astype(np.float32)
    out.append(("signed_zero", x2, z, int(x2.sum())))
    out.append(("constant", x, np.full(vox, 0.25, np.float32), int(x.sum())))
    x3 = np.zeros(vox, np.float32)
    x3[int(rng.integers(vox))] = 1
    out.append(("n1", x3, rng.standard_normal(vox).astype(np.float32), 1))
    out.append(("distinct", x2, rng.standard_normal(vox).astype(np.float32), int(x2.sum())))
    return [(n_, a.reshape(cs, cs, cs), b.reshape(cs, cs, cs), c) for n_, a, b, c in out]


def big_k_cube(seed=6):
    """a 64^3 cube whose stored count asks for K = 65535 (3 n > 65535) with three occupied voxels"""
    rng = np.random.default_rng(seed)
    x = np.zeros(64 ** 3, np.float32)
    x[rng.choice(64 ** 3, 3, replace=False)] = 1
    logits = rng.standard_normal(64 ** 3).astype(np.float32)
    return x.reshape(64, 64, 64), logits.reshape(64, 64, 64), 30000


def test_candidate_counts():
    assert list(pn.candidate_counts([0, 1, 5, 21845, 21846, 65535], 64 ** 3)) == [1, 3, 15, 65535, 65535, 65535]
    assert list(pn.candidate_counts([100, 200], 512)) == [300, 512]          # never more than the cube holds


def test_ladder_counts_match_select_voxels():
    n = np.array([1, 7, 333, 4096], np.uint16)
    K = pn.candidate_counts(n, 64 ** 3)
    lad = pn.ladder_counts(n, K, pn.RHOS_D1)
    for i, rho in enumerate(pn.RHOS_D1):
        want = [min(max(int(rho * np.array(v)), 1), k) for v, k in zip(n, K)]
        assert list(lad[i]) == want
    assert list(lad[pn.RHOS_D1.index(1.0)]) == [int(v) for v in n]          # rho = 1: today's counts


@pytest.mark.parametrize("case", range(5))
def test_restatement_equals_direct_masks(case):
    name, x, l, n = engineered_cubes()[case]
    m, A, B = ref.curves_ref(x, l, n)
    K = int(pn.candidate_counts([n], x.size)[0])
    assert len(m) == len(A) == len(B) == K
    direct = ref.curves_direct(x, l, range(1, K + 1))
    assert [tuple(int(v) for v in t) for t in zip(m, A, B)] == direct, name
    if name == "constant":
        assert (m == x.size).all()


def test_restatement_big_k():
    x, l, n = big_k_cube()
    m, A, B = ref.curves_ref(x, l, n)
    assert len(m) == 65535
    ks = [1, 2, 100, 4097, 65534, 65535]
    assert [(int(m[k - 1]), int(A[k - 1]), int(B[k - 1])) for k in ks] == ref.curves_direct(x, l, ks)


def _sums(ks_row, curves):
    s = [0, 0, 0]
    for b, (m, A, B) in enumerate(curves):
        k = ks_row[b] - 1
        s[0] += int(A[k]); s[1] += int(B[k]); s[2] += int(m[k])
    return s


def test_selection_tie_rules():
    rhos = [0.8, 1.0, 1.2]
    same = (10, 20, 5)
    kind, i, f = pn.select_assignment([same, same], [same, same, same], rhos, 2)
    assert (kind, i) == ("ladder", 1) and f == Fraction(5)                 # rho = 1 first
    better = (8, 20, 5)
    kind, i, _ = pn.select_assignment([better, better], [same, better, better], [1.0, 0.8, 1.2], 2)
    assert (kind, i) == ("ladder", 1)                                      # then the ladder in order
    kind, i, _ = pn.select_assignment([same, better, better], [same], [1.0], 2)
    assert (kind, i) == ("sweep", 1)                                       # then ascending j
    # exact comparison: 10**17 / (3 10**17 + 1) < 1/3 although the two are equal as doubles
    big = 3 * 10 ** 17
    assert float(Fraction(10 ** 17, big + 1)) == 1 / 3
    kind, i, f = pn.select_assignment([(10 ** 17, 0, 1)], [(0, 1, 3)], [1.0], big + 1)
    assert (kind, i) == ("sweep", 0) and f == Fraction(10 ** 17, big + 1)


@pytest.mark.parametrize("seed", range(4))
def test_guarantees_on_random_curves(seed):
    rng = np.random.default_rng(seed)
    curves, nums = [], []
    for _ in range(int(rng.integers(3, 9))):
        n = int(rng.integers(1, 40))
        K = 3 * n
        m = np.cumsum(rng.integers(1, 3, K))
        A = np.sort(rng.integers(0, 10 * n, K))[::-1].copy()              # fewer misses as S grows
        B = np.cumsum(rng.integers(0, 6, K))
        curves.append((m, A, B))
        nums.append(n)
    nums = np.array(nums)
    K = np.array([len(c[0]) for c in curves])
    lad = pn.ladder_counts(nums, K, pn.RHOS_D1)
    ks, sums = ref.sweep_ref(curves, 64, lad)
    sum_n = int(nums.sum())
    sweep_sums = [tuple(int(v) for v in s) for s in sums[:65]]
    ladder_sums = [tuple(int(v) for v in s) for s in sums[65:]]
    assert ladder_sums == [tuple(_sums(lad[i], curves)) for i in range(len(pn.RHOS_D1))]
    kind, i, f = pn.select_assignment(sweep_sums, ladder_sums, pn.RHOS_D1, sum_n)
    for s in ladder_sums + sweep_sums:
        assert f <= pn.cloud_f(s[0], sum_n, s[1], s[2])
    count = ladder_sums[pn.RHOS_D1.index(1.0)]
    assert f <= pn.cloud_f(count[0], sum_n, count[1], count[2])


def test_pointnums_flag():
    from pcgcv1_amd import test as cli
    assert cli.parse_args(["compress", "x.ply"]).pointnums == "count"
    assert cli.parse_args(["compress", "x.ply", "--pointnums", "d1"]).pointnums == "d1"
    with pytest.raises(SystemExit):
        cli.parse_args(["compress", "x.ply", "--pointnums", "d2"])
    assert any(f[0] == "pointnums" for f in cli._FLAGS)


def test_eval_pointnums_flag():
    import inspect
    from pcgcv1_amd import eval as rd
    from pcgcv1_amd import eval_ablation_studies as ab
    assert inspect.signature(rd.eval).parameters["pointnums"].default == "count"
    assert inspect.signature(rd.rate_point).parameters["pointnums"].default == "count"
    assert inspect.signature(ab.eval).parameters["pointnums"].default == "count"


def test_sharded_refuses_d1():
    from pcgcv1_amd import test as cli
    with pytest.raises(SystemExit, match="pointnums"):
        cli.main(["compress", "x.ply", "--gpu", "2", "--pointnums", "d1"])
