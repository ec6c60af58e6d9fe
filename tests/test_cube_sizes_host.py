"""What the inputs of test_gpu_cube_sizes.py (tests/_cube_sizes.py) are for, on the CPU oracle alone.

The entropy-stage test codes five of the seven cubes at 32 and 16.  The container holds |min|, |max| <= 15 per stream and the
quantiser needs at least two symbols (synthetic.py header), so those cubes must keep their rounded latents inside that and
the two left out must be left out for the reason given.  Measured with the oracle (y per cube; z of the seven-cube batch):

  cube size   sheet 0     sheet 1     sheet 2     empty     corners   faces      30 %        z
  32          [-13, 10]   [-14, 13]   [-15, 12]   [-1, 1]   [-1, 1]   [-10, 8]   [-33, 23]   [-8, 11]
  16          [-10, 7]    [-9, 8]     [-11, 10]   [-1, 1]   [-1, 1]   [-11, 8]   [-20, 16]   [-2, 2]
"""
import numpy as np
import pytest

pytest.importorskip("torch")

import _cube_sizes as cz       # noqa: E402

LIMIT = 14                      # one inside the container's 15: the HIP latents differ from the oracle's in the last bits


def _range(a):
    r = np.rint(a)
    return int(r.min()), int(r.max())


@pytest.mark.parametrize("cs", [16, 32, 96])
def test_batch_is_what_the_docstring_says(cs):
    x = cz.batch(cs)
    assert x.shape == (cz.N_CUBES, cs, cs, cs, 1) and x.dtype == np.float32 and set(np.unique(x)) <= {0.0, 1.0}
    assert not x.flags.writeable and cz.batch(cs) is x                       # computed once, shared, left unchanged
    v = x[..., 0]
    faces = lambda c: [bool(c[0].any()), bool(c[-1].any()), bool(c[:, 0].any()), bool(c[:, -1].any()),       # noqa: E731
                       bool(c[:, :, 0].any()), bool(c[:, :, -1].any())]                                      # d, h, w: first, last
    # the three sheets lie across d, h and w: together they reach every face of the cube
    assert all(np.logical_or.reduce([faces(v[i]) for i in cz.SHEETS]))
    for i in cz.SHEETS:
        assert 0.02 * cs ** 3 < v[i].sum() <= 0.03 * cs ** 3 + cs * cs
    assert not v[cz.EMPTY].any()
    assert sorted(map(tuple, np.argwhere(v[cz.CORNERS]))) == [(0, 0, 0), (0, cs - 1, 0), (cs - 1, cs - 1, cs - 1)]
    # the face cube: the planes w = 0, w = cs-1, d = 0 and h = cs-1 are full, nothing lies off them, h = 0 and d = cs-1 are not full
    f = v[cz.FACES]
    assert f[:, :, 0].all() and f[:, :, -1].all() and f[0].all() and f[:, -1].all()
    assert not f[1:, :-1, 1:-1].any() and not f[:, 0].all() and not f[-1].all()
    assert int(f.sum()) == cs ** 3 - (cs - 1) * (cs - 1) * (cs - 2)
    assert abs(v[cz.RANDOM].mean() - 0.3) < 4 * np.sqrt(0.3 * 0.7 / cs ** 3)          # four standard deviations
    assert np.array_equal(v[cz.RANDOM], np.random.default_rng(3).random((cs, cs, cs)) < 0.3)


@pytest.mark.parametrize("cs", [32, 16])
def test_latent_ranges_make_the_entropy_test_legal(cs):
    y, z = cz.oracle_y(cs, cz.N_CUBES), cz.oracle_z(cs, cz.N_CUBES)
    assert y.shape == (cz.N_CUBES, cs // 4, cs // 4, cs // 4, 16) and z.shape == (cz.N_CUBES, cs // 8, cs // 8, cs // 8, 8)
    ranges = [_range(y[b]) for b in range(cz.N_CUBES)]
    print("cube size %d: y per cube %s, z of the batch %s" % (cs, ranges, _range(z)))
    for b in cz.RANGE_SAFE:
        lo, hi = ranges[b]
        assert -LIMIT <= lo <= 0 <= hi <= LIMIT and hi - lo >= 1, (cs, b, lo, hi)
    # z is one stream per batch: of the seven cubes and of the five the entropy test codes
    for zz in (z, z[list(cz.RANGE_SAFE)]):
        lo, hi = _range(zz)
        assert -LIMIT <= lo <= 0 <= hi <= LIMIT and hi - lo >= 1, (cs, lo, hi)
    # the all-zero cube's latents are not all zero (biases), so even it has two symbols; the corner cube differs from it
    assert not np.array_equal(y[cz.EMPTY], y[cz.CORNERS])
    # why the other two cubes are left out: at 32 the third sheet reaches the container's limit, the 30 % cube is far outside
    if cs == 32:
        assert max(map(abs, ranges[cz.SHEETS[2]])) > LIMIT
    assert max(map(abs, ranges[cz.RANDOM])) > 15


def test_references_are_cached_and_frozen():
    y = cz.oracle_y(16, cz.N_CUBES)
    assert cz.oracle_y(16, cz.N_CUBES) is y and not y.flags.writeable
    loc, scale = cz.oracle_loc_scale(16, cz.N_CUBES)
    assert loc.shape == y.shape and scale.shape == y.shape and float(scale.min()) >= 1e-9
    assert cz.oracle_x(16, cz.N_CUBES).shape == (cz.N_CUBES, 16, 16, 16, 1)
