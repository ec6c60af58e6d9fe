"""What the inputs of test_gpu_entropy_forms.py (tests/_entropy_cases.py) are for, on the CPU oracle alone.

The Laplace CDF launches must reach every instantiation of laplace_cdf_kernel at both ends of its ncols interval, both
directions of the integer correction, its bulk step (deficits in the thousands), exactly tied keys, segments narrower than the
row stride and both ends of every symbol range — and must stay cheap for the oracle's step-by-step quantiser."""
import time

import numpy as np
import pytest

pytest.importorskip("torch")

import _entropy_cases as ec       # noqa: E402
from oracle import entropy as oent       # noqa: E402

LAUNCHES = ec.CDF_NCOLS + (ec.ROWWISE,)


def test_every_instantiation_is_reached_at_both_ends_of_its_interval():
    assert [(n, ec.cdf_instantiation(n)) for n in ec.CDF_NCOLS] == [
        (2, 4), (3, 4), (4, 4), (5, 8), (8, 8), (9, 16), (16, 16), (17, 32), (31, 32), (32, 32)]
    assert ec.cdf_instantiation(1) == 4 and ec.cdf_instantiation(ec.cdf_case(ec.ROWWISE)["ncols"]) == 8
    for maxn, lo in ((4, 2), (8, 5), (16, 9), (32, 17)):        # lo: the narrowest ncols of <MAXN> that a test can give a narrower segment
        mine = [n for n in ec.CDF_NCOLS if ec.cdf_instantiation(n) == maxn]
        assert min(mine) == lo and max(mine) == maxn


@pytest.mark.parametrize("name", LAUNCHES)
def test_cdf_launch_is_what_the_tests_need(name):
    c = ec.cdf_case(name)
    assert ec.cdf_case(name) is c and not c["loc"].flags.writeable                   # computed once, shared, left unchanged
    rows, seg_rows, ncols = c["rows"], c["seg_rows"], c["ncols"]
    mn, mx = c["row_min"], c["row_max"]
    width = mx - mn + 1
    assert rows % seg_rows == 0 and c["seg_min"].size == rows // seg_rows
    assert mn.min() >= -16 and mx.max() <= 16 and width.max() <= ncols and width.min() >= 1
    assert (width < ncols).any()                                                      # 0xFFFF columns are written
    if name == ec.ROWWISE:
        assert rows == 1000 and rows % 256 != 0 and seg_rows == 1 and sorted(set(width)) == [2, 3, 4, 5, 6, 7, 8]
    else:
        assert seg_rows == 1024 and sorted(set(width)) == sorted({ncols, 2, ncols // 2 + 1, 1})
        full = [(int(a), int(b)) for a, b in zip(c["seg_min"], c["seg_max"]) if b - a + 1 == ncols]
        assert any(a < 0 < b or (a, b) == (-1, 0) for a, b in full) and (len(full) == 2 or ncols == 2)
        assert any(a == 0 or b == 16 for a, b in full)                                # one-sided: touching 0, or as far as 16 allows
    assert (c["scale"] > 0).all() and np.isfinite(c["loc"]).all()
    for v in (1e-9, 1e-4, 0.3, 7.0, 100.0, 1e4):
        assert (c["scale"] == np.float32(v)).any()
    # both directions of the correction and its bulk step
    deficit = ec.row_deficits(c["loc"], c["scale"], mn, mx)
    assert (deficit > 1000).sum() >= 32 and (deficit < 0).sum() >= 8, ((deficit > 1000).sum(), (deficit < 0).sum())
    # slow rows are capped per block of 1024 rows
    slow = deficit > ec.SLOW_DEFICIT
    per_block = [int(slow[s:s + ec.SEG_ROWS].sum()) for s in range(0, rows, ec.SEG_ROWS)]
    assert max(per_block) <= ec.SLOW_CAP, per_block
    assert slow.any()                                                                 # ... not removed: the long runs stay covered
    # exactly tied keys: loc = 0 in a range symmetric about 0 gives a mirror-symmetric pmf, and the correction has work to do
    tied = 0
    for (a, b), i in ec._groups(mn, mx):
        if a == -b and b > 0:
            j = i[(c["loc"][i] == 0) & (deficit[i] != 0)]
            pmf = oent.sc_pmf(c["loc"][j, None], c["scale"][j, None], a, b)[:, 0, :]
            assert np.array_equal(pmf.view(np.uint32), pmf[:, ::-1].view(np.uint32))
            tied += j.size
    # (few where the ranges are narrow: sign(2q - loc) = 0 leaves the symbol 0 of such a row the bound's 1e-9, its mass must lie
    # in the tails, and a row that keeps less than 0.69 inside its range is a slow one)
    if ncols > 2:
        assert tied >= 8, tied
    # ... and the same about a range's own axis, the only kind a launch of ncols = 2 can hold ([-1, 0] about -0.5).  Counted,
    # not demanded of every such row: sign(2q - loc) reflects the symbols between loc / 2 and loc to the wrong side, so about
    # a positive axis the two tails differ in the last bit
    tied_axis = 0
    for (a, b), i in ec._groups(mn, mx):
        if b > a:
            j = i[(c["loc"][i] == np.float32((a + b) * 0.5)) & (deficit[i] != 0)]
            pmf = oent.sc_pmf(c["loc"][j, None], c["scale"][j, None], a, b)[:, 0, :]
            tied_axis += int((pmf.view(np.uint32) == pmf[:, ::-1].view(np.uint32)).all(1).sum())
    assert tied_axis >= 16, tied_axis
    # symbols: integers inside the range, reaching both of its ends in every segment
    sym = c["symbols"]
    assert sym.dtype == np.float32 and np.array_equal(sym, np.rint(sym)) and (sym >= mn).all() and (sym <= mx).all()
    if name == ec.ROWWISE:
        assert (sym == mn).sum() >= 32 and (sym == mx).sum() >= 32
    else:
        s = sym.reshape(-1, seg_rows)
        assert np.array_equal(s.min(1), c["seg_min"]) and np.array_equal(s.max(1), c["seg_max"])


def test_references_are_cheap_and_well_formed(capsys):
    """The CPU share of the whole GPU file: every reference once.  The cap on slow rows is what keeps the oracle's
    step-by-step quantiser out of the tens of seconds (8 segments of 2048 uncapped rows: 8 to 13 s per width)."""
    t0 = time.perf_counter()
    for name in LAUNCHES:
        c = ec.cdf_case(name)
        cdf, lohi = ec.cdf_reference(name)
        width = c["row_max"] - c["row_min"] + 1
        k = np.arange(c["ncols"])[None, :]
        assert cdf.shape == (c["rows"], c["ncols"]) and (cdf[:, 0] == 0).all() and (cdf[k >= width[:, None]] == 0xFFFF).all()
        inside = np.where(k < width[:, None], cdf.astype(np.int64), 65536 + k)
        assert (np.diff(inside, axis=1) > 0).all()                                    # every symbol keeps at least one count
        lo, hi = (lohi & 0xFFFF).astype(np.int64), (lohi >> 16).astype(np.int64)
        assert (lo <= hi).all()
        ks = (c["symbols"] - c["row_min"]).astype(np.int64)
        assert np.array_equal(lo, cdf[np.arange(c["rows"]), ks])
        assert (hi[ks == width - 1] == 65535).all()
    t_cdf = time.perf_counter() - t0
    with capsys.disabled():
        print("\noracle CDF rows of %d launches: %.1f s" % (len(LAUNCHES), t_cdf))
