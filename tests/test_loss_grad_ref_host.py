"""The reference of tests/test_gpu_train_loss.py checked on its own, without a GPU: the float64 autograd gradients against
central finite differences, the seeded generators against the bins they claim and the margins they promise, and the float32
CPU evaluation (the yardstick of the comparison rule) for finiteness."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import _loss_grad_ref as R                     # noqa: E402
from oracle import train as otrain             # noqa: E402

F64 = torch.float64
H = 1e-5


def _close(fd, g, what):
    """relative 1e-6 on the rule's own element scale (|g| plus 1e-3 of the largest |g|)."""
    e = R.err(fd, g, R.elem_scale(g))
    assert e <= 1e-6, (what, e)


def _laplace_logp(y, loc, scale):
    t = [torch.from_numpy(np.asarray(v, np.float64)) for v in (y, loc, scale)]
    return torch.log(torch.clamp_min(otrain._sc_likelihood(*t), R.BOUND)).numpy()


def test_laplace_float64_gradients_match_finite_differences():
    rng = np.random.default_rng(1)
    n = 400
    loc = np.float32(2.0 * rng.standard_normal(n))
    scale = np.float32(rng.uniform(0.5, 2.0, n))
    y = np.float32(loc + scale * rng.uniform(-3.0, 3.0, n))
    # well-conditioned: away from the kinks of |x - loc| at both edges and of sign(2v - loc)
    ok = (np.abs(y + 0.5 - loc) > 0.01) & (np.abs(y - 0.5 - loc) > 0.01) & (np.abs(2.0 * y - loc) > 0.01)
    y, loc, scale = y[ok], loc[ok], scale[ok]
    assert y.size >= 300
    coef = -0.37
    dy, dloc, dscale, p = R.laplace_grad(y, loc, scale, coef)
    assert p.min() > 1e-4
    c = float(np.float32(coef))
    y64, l64, s64 = (np.asarray(v, np.float64) for v in (y, loc, scale))
    _close(c * (_laplace_logp(y64 + H, l64, s64) - _laplace_logp(y64 - H, l64, s64)) / (2 * H), dy, "dy")
    _close(c * (_laplace_logp(y64, l64 + H, s64) - _laplace_logp(y64, l64 - H, s64)) / (2 * H), dloc, "dloc")
    _close(c * (_laplace_logp(y64, l64, s64 + H) - _laplace_logp(y64, l64, s64 - H)) / (2 * H), dscale, "dscale")


def _fz_logp(z, w):
    C = w["estimator/matrix_0"].shape[0]
    wt = {k: torch.from_numpy(np.asarray(v, np.float64)) for k, v in w.items()}
    t = torch.from_numpy(np.asarray(z, np.float64).reshape(-1, C).T.reshape(1, C, -1, 1, 1).copy())
    p = otrain._eb_likelihood(wt, t)
    return torch.log(torch.clamp_min(p, R.BOUND)).numpy().reshape(C, -1).T.ravel()


def test_factorized_float64_gradients_match_finite_differences():
    C, m = 8, 48
    w = R.eb_weights(C, perturbed=True)
    z = np.float32(2.0 * np.random.default_rng(2).standard_normal(m * C))
    coef = -0.37
    c = float(np.float32(coef))
    dz, dparams, p = R.factorized_grad(z, w, coef)
    assert p.min() > 1e-6
    z64 = np.asarray(z, np.float64)
    _close(c * (_fz_logp(z64 + H, w) - _fz_logp(z64 - H, w)) / (2 * H), dz, "dz")
    # several of the 44 * C parameters: four entries of each of the twelve tensors, channels spread over all eight
    g = R.unpack_params(dparams, C)
    rng = np.random.default_rng(3)
    for name in g:
        flat = g[name].ravel()
        scale = float(np.abs(flat).max())
        for idx in rng.choice(flat.size, 4, replace=False):
            fd = 0.0
            for sgn in (1.0, -1.0):
                w2 = {k: np.asarray(v, np.float64).copy() for k, v in w.items()}
                w2[name].reshape(-1)[idx] += sgn * H
                fd += sgn * c * _fz_logp(z64, w2).sum()
            fd /= 2 * H
            assert abs(fd - flat[idx]) <= 1e-6 * scale, (name, idx, fd, flat[idx], scale)


def test_pack_and_unpack_are_inverse_and_follow_the_packed_order():
    for C in (1, 8, 32):
        w = R.eb_weights(C, perturbed=True)
        vec = R.pack_params(w)
        assert vec.shape == (44 * C,)
        back = R.unpack_params(vec, C)
        assert list(back) == ["estimator/" + n for n in R.EB_NAMES]
        for k in back:
            assert back[k].shape == w[k].shape and np.array_equal(back[k], w[k]), k
        assert np.array_equal(vec[:3 * C], w["estimator/matrix_0"].ravel())
        assert np.array_equal(vec[-C:], w["estimator/factor_3"].ravel())


def test_bce_float64_gradient_matches_finite_differences():
    rng = np.random.default_rng(4)
    n = 400
    pred = np.float32(rng.uniform(-8.0, 8.0, n))
    label = np.float32(R.BCE_LABELS)[rng.integers(0, 5, n)]
    c0, c1 = np.float32(0.31), np.float32(0.011)
    g, _ = R.bce_grad(pred, label, c0, c1)

    def loss(x):
        o = np.clip(1.0 / (1.0 + np.exp(-x)), 1e-7, 1.0 - 1e-7)
        return np.where(label == 0, -float(c0) * np.log(1.0 - o), np.where(label > 0, -float(c1) * np.log(o), 0.0))
    x = np.asarray(pred, np.float64)
    _close((loss(x + H) - loss(x - H)) / (2 * H), g, "dpred")
    assert np.all(g[label < 0] == 0)


def test_laplace_wide_edge_elements_sit_on_loc_and_are_well_conditioned():
    y, loc, scale = R.engineered_laplace_edge_wide()
    assert np.all((y + np.float32(0.5) == loc) | (y - np.float32(0.5) == loc)) and (y - np.float32(0.5) == loc).sum() == 2
    g64, g32 = R.laplace_grad(y, loc, scale, -1.0), R.laplace_grad(y, loc, scale, -1.0, torch.float32)
    assert g64[3].min() > 0.1 and np.all(g64[0] != 0) and np.all(g64[2] != 0)
    for a, b in zip(g32[:3], g64[:3]):                      # float32 autograd itself is within 1e-6: 1e-5 leaves the kernel room
        assert np.all(np.abs(a - b) <= 1e-6 * np.abs(b))


@pytest.mark.parametrize("regime", R.LAPLACE_REGIMES)
def test_laplace_generators_fill_their_bins_and_keep_their_margins(regime):
    y, loc, scale, claims = R.gen_laplace(regime)
    assert y.size == R.N_BIG and y.dtype == loc.dtype == scale.dtype == np.float32
    assert np.all(scale >= np.float32(1e-9))
    g64 = R.laplace_grad(y, loc, scale, -1.0)
    counts = [int(m.sum()) for m in R.bin_masks(g64[3], R.LAPLACE_BINS)]
    for k in claims:
        assert counts[k] >= R.MIN_BIN, (regime, counts)
    assert np.all(R.margin_laplace(y, loc, scale, g64[3]))
    g32 = R.laplace_grad(y, loc, scale, -1.0, torch.float32)
    assert all(np.isfinite(a).all() for a in g32 + g64)
    if regime == "flip":          # both edges beyond loc, on the far side from 0
        assert np.all(np.abs(y) < np.abs(loc)) and np.all(2 * np.abs(y) > np.abs(loc)) and (loc > 0).any() and (loc < 0).any()
    if regime == "tail":          # float32 stays accurate down to the floor: the regime that shows a wrong floor
        m = R.bin_masks(g64[3], R.LAPLACE_BINS)[3]
        assert R.err(g32[0][m], g64[0][m], R.elem_scale(g64[0][m])) < 1e-3


def test_laplace_engineered_elements_are_what_they_claim():
    y, loc, scale = R.engineered_laplace_zero()
    for dtype in (F64, torch.float32):
        g = R.laplace_grad(y, loc, scale, -1.0, dtype)
        assert all(np.all(a == 0) for a in g[:3]) and np.isfinite(g[3]).all()
    assert (2 * y == loc).sum() >= 3 and (np.abs(y - loc) / scale >= 200).sum() >= 6 and (scale == np.float32(1e-9)).sum() >= 4
    y, loc, scale = R.engineered_laplace_edge()
    assert np.all(y + np.float32(0.5) == loc) and np.all(scale == np.float32(1e-9))
    for dtype in (F64, torch.float32):
        g = R.laplace_grad(y, loc, scale, -1.0, dtype)
        assert all(np.isfinite(a).all() for a in g) and np.all(g[3] == 0.5)


def test_bce_generator_fills_its_bins_and_keeps_its_margin():
    pred, label = R.gen_bce()
    assert pred.size == R.N_BIG
    f = R.bce_factor(pred, label)
    for k, m in enumerate(R.bin_masks(f, R.BCE_BINS)):
        assert int((m & (label == 0)).sum()) >= R.MIN_BIN and int((m & (label > 0)).sum()) >= R.MIN_BIN, k
    assert np.all(R.margin_bce(pred))
    o = 1.0 / (1.0 + np.exp(-np.asarray(pred, np.float64)))
    assert o.min() >= 2 * R.CLIP * (1 - 1e-6) and (1 - o).min() >= 2 * R.CLIP * (1 - 1e-6)
    assert set(np.unique(label)) == set(R.BCE_LABELS)
    g32, _ = R.bce_grad(pred, label, 0.3, 0.7, torch.float32)
    assert np.isfinite(g32).all()
    pe, le, inside = R.engineered_bce()
    for dtype in (F64, torch.float32):
        g, _ = R.bce_grad(pe, le, 0.3, 0.7, dtype)
        assert np.isfinite(g).all() and np.all(g[~inside] == 0) and np.all(g[le < 0] == 0)
        assert np.all(g[inside & (le >= 0)] != 0)          # +-16.0 is inside the clip: the full value, in both precisions


@pytest.mark.parametrize("C", R.FZ_CHANNELS)
def test_factorized_generator_fills_its_bins_and_keeps_its_margin(C):
    for kind, pert in R.FZ_KINDS:
        w = R.eb_weights(C, pert)
        m = R.fz_m(C, kind)
        for draw in range(1, R.FZ_DRAWS_ONE if m == 1 else 1):
            zd, _ = R.gen_factorized(C, m, w, seed=draw)
            pd = R.factorized_grad(zd, w, -1.0)[2]
            assert np.all((pd < R.BOUND / 2) | (pd > 2 * R.BOUND))
            assert all(np.isfinite(a).all() for a in R.factorized_grad(zd, w, -1.0, torch.float32))
        z, eng = R.gen_factorized(C, m, w)
        assert z.size == m * C and z.dtype == np.float32
        dz, dparams, p = R.factorized_grad(z, w, -1.0)
        assert np.all((p < R.BOUND / 2) | (p > 2 * R.BOUND))
        r32 = R.factorized_grad(z, w, -1.0, torch.float32)
        assert all(np.isfinite(a).all() for a in r32) and np.isfinite(dz).all() and np.isfinite(dparams).all()
        if m > 1:
            # the +-1000 sit below the floor for every weight set (at +-60 these synthetic tails still hold p up to 6e-3)
            far = np.abs(z) == 1000
            assert far.sum() >= 4 and np.all(p[far] < R.BOUND / 2) and np.all(dz[far] == 0) and (np.abs(z) == 60).sum() >= 2
            assert sum(int(mk.sum()) >= R.MIN_BIN for mk in R.bin_masks(p, R.FZ_BINS)) >= 1
        if pert and C > 1:
            a = w["estimator/matrix_1"].reshape(C, -1)
            assert len(np.unique(a, axis=0)) == C          # no two channels alike


@pytest.mark.parametrize("lb", [1e-9, 0.11])
def test_abs_max_generator_and_formulas(lb):
    s, dscale, k = R.gen_abs_max(lb, 4096)
    assert k == 8 and np.all(R.margin_abs_max(s[k:], lb))
    l32 = np.float32(lb)
    assert s[2] == l32 and s[3] == -l32 and abs(s[4]) > l32 > abs(s[6]) and np.signbit(s[1]) and s[1] == 0
    out = R.abs_max_bwd(dscale, s, lb)
    assert out[2] == dscale[2] and out[3] == -dscale[3] and out[4] == dscale[4] and out[6] == 0 and out[7] == 0      # tie goes to |s|
    assert out[0] == 0 and out[1] == 0
    assert (np.abs(s) >= l32).sum() >= R.MIN_BIN and (np.abs(s) < l32).sum() >= R.MIN_BIN
    assert np.array_equal(R.abs_max_fwd(s, lb), np.where(np.abs(s) >= l32, np.abs(s), l32))


def test_relu_reference_slices_and_masks():
    dy, y = R.gen_relu(5, 8, 16)
    out = R.relu_bwd(dy, 16, 8, y, 5, 8).reshape(5, 8)
    yy, dd = y.reshape(5, 8), dy.reshape(5, 16)
    for v in range(5):
        for c in range(8):
            assert out[v, c] == (dd[v, 8 + c] if yy[v, c] > 0 else 0)
    assert np.array_equal(R.relu_bwd(dy, 16, 0, None, 5, 8).reshape(5, 8), dd[:, :8])
    assert (y == 0).sum() >= 2 and ((y != 0) & (np.abs(y) < 1e-38)).sum() >= 4
