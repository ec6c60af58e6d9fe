"""Reference for the rate and loss reverse kernels of csrc/train.hip.  Plain numpy / torch on the CPU, no GPU.

The gradients come from torch autograd through the oracle's own forward functions (oracle/train.py: _sc_likelihood,
_eb_likelihood and the BCE lines of forward_loss); nothing here restates the kernels' closed-form gradients.  Every
function takes a dtype: torch.float64 is the reference, torch.float32 is the yardstick of what float32 can deliver for the
same formula.  Both are fed the SAME float32 inputs, so rounding of the inputs is no error source.

Comparison rule (compare()): for one output and one bin,  E(g) = max_i |g_i - g64_i| / S_i  with S from float64:
    element outputs       S_i = |g64_i| + 1e-3 * (largest |g64| of the bin)
    parameter gradients   S   = largest |g64| of the tensor
and the kernel passes when  E(kernel) <= 4 * E(float32 CPU autograd) + 16 * 2^-24.  The two float32 evaluations differ by
their exp / tanh / log1p implementations (a few ulp each) and by summation order, and both go through the same
amplification (the cancellation of the two CDF values at small likelihood): on the CPU their ratio was at most 1.3 per bin,
a wrong sign, factor or index gives E near 1.  The limit always comes from the reference pair, never from the kernel.

Decision thresholds.  float32 and float64 may take different sides of a branch when an input sits on it, so the seeded
generators keep every random element a factor 2 away (margin_*()): the likelihood p64 from its bound, the sigmoid from its
clip, |s| from the lower bound, and 2v - loc (values of order 1 to 10, float32 spacing 1e-6) at least 1e-3 from 0.
Offending draws are replaced by a harmless element, so sizes stay exact.  Elements placed ON a threshold on purpose are
kept apart (engineered_*()) and checked exactly.

TensorFlow tie conventions: tf.maximum passes the gradient where x >= y (torch.maximum splits a tie), so max(|s|, lb) has a
numpy formula here and not autograd; clip_by_value and tf.maximum(p, bound) pass it on the closed interval, as torch.clamp
does.
"""
import numpy as np
import torch

from oracle import train as otrain
from pcgcv1_amd.train_hyper import EB_NAMES

BOUND = 1e-9                     # likelihood floor of both entropy models
CLIP = 1e-7                      # sigmoid clip of the BCE
LN2 = float(np.log(2.0))
SLACK = 16 * 2.0 ** -24
N_BIG = 4096 * 256 + 333         # grid_for caps at 4096 blocks of 256: the last 333 elements need a second trip
_CHUNK = 1 << 17                 # elements per autograd call (memory); gradients of a sum of per-element terms add up

LAPLACE_REGIMES = ("typical", "wide", "flip", "tail")
LAPLACE_BINS = ((1e-2, 1.0 + 1e-9), (1e-4, 1e-2), (1e-6, 1e-4), (1e-8, 1e-6))
BCE_BINS = tuple((10.0 ** -(k + 1), 10.0 ** -k if k else 1.0 + 1e-9) for k in range(7))
FZ_BINS = tuple((10.0 ** -(k + 1), 10.0 ** -k if k else 1.0 + 1e-9) for k in range(8))
MIN_BIN = 200


def _f32(a):
    return np.ascontiguousarray(a, np.float32)


def _leaf(a, dtype):
    return torch.from_numpy(_f32(a)).to(dtype).requires_grad_(True)


# ------------------------------------------------------------------ comparison rule
def bin_masks(key64, bins):
    return [(key64 >= lo) & (key64 < hi) for lo, hi in bins]


def elem_scale(g64):
    g64 = np.abs(np.asarray(g64, np.float64))
    return g64 + 1e-3 * (g64.max() if g64.size else 0.0)


def err(g, g64, scale):
    """E(g) of the rule; scale an array (element outputs) or a number (parameter gradients)."""
    g, g64 = np.asarray(g, np.float64), np.asarray(g64, np.float64)
    if g.size == 0:
        return 0.0
    d = np.abs(g - g64)
    if not np.all(np.isfinite(d)):
        return float("inf")
    if np.ndim(scale) == 0:
        return float(d.max() / scale) if scale > 0 else (0.0 if d.max() == 0 else float("inf"))
    ok = scale > 0
    if np.any(d[~ok] != 0):
        return float("inf")
    return float((d[ok] / scale[ok]).max()) if ok.any() else 0.0


def err_pair(g_kernel, g32, g64, param=False):
    g64 = np.asarray(g64, np.float64)
    scale = float(np.abs(g64).max()) if param else elem_scale(g64)
    return err(g_kernel, g64, scale), err(g32, g64, scale)


def judge(what, n, ek, e32, log=print):
    """The rule's verdict on one bin; prints both E values."""
    log("%-46s n=%-8d E(kernel)=%.3g  E(float32 cpu)=%.3g" % (what, n, ek, e32))
    assert ek <= 4.0 * e32 + SLACK, "%s: E(kernel)=%.4g > 4 * %.4g + %.3g" % (what, ek, e32, SLACK)
    return ek, e32


def compare(what, g_kernel, g32, g64, param=False, log=print):
    """Apply the rule to one bin."""
    return judge(what, np.size(g64), *err_pair(g_kernel, g32, g64, param), log=log)


# ------------------------------------------------------------------ Laplace likelihood
def laplace_grad(y, loc, scale, coef, dtype=torch.float64, bound=BOUND):
    """Gradients of coef * sum(log(max(p, bound))), p = oracle.train._sc_likelihood -> (dy, dloc, dscale, p)."""
    y, loc, scale = _f32(y), _f32(loc), _f32(scale)
    c = float(np.float32(coef))
    outs = [[], [], [], []]
    for a in range(0, y.size, _CHUNK):
        ty, tl, ts = (_leaf(v[a:a + _CHUNK], dtype) for v in (y, loc, scale))
        p = otrain._sc_likelihood(ty, tl, ts)
        (c * torch.log(torch.clamp_min(p, bound)).sum()).backward()
        for o, t in zip(outs, (ty.grad, tl.grad, ts.grad, p.detach())):
            o.append(t.numpy())
    return tuple(np.concatenate(o) for o in outs)


def margin_laplace(y, loc, scale, p64):
    """True where a random element keeps clear of the kernel's decisions: the floor and the sign(2v - loc) flip."""
    y, loc = np.asarray(y, np.float64), np.asarray(loc, np.float64)
    return ((p64 < BOUND / 2) | (p64 > 2 * BOUND)) & (np.abs(2 * y - loc) >= 1e-3)


def _laplace_clean(y, loc, scale, safe=(0.25, 0.0, 1.0)):
    y, loc, scale = _f32(y), _f32(loc), _f32(scale)
    p64 = laplace_grad(y, loc, scale, 1.0)[3]
    bad = ~margin_laplace(y, loc, scale, p64)
    y[bad], loc[bad], scale[bad] = safe
    return y, loc, scale


def gen_laplace(regime, n=N_BIG, seed=0):
    """-> (y, loc, scale) float32 and the tuple of LAPLACE_BINS indices the regime claims to fill."""
    rng = np.random.default_rng(1000 + seed + {"typical": 0, "wide": 1, "flip": 2, "tail": 3}[regime])
    if regime == "typical":
        loc = 0.7 * rng.standard_normal(n)
        scale = np.maximum(0.8 * np.abs(rng.standard_normal(n)), 1e-9)
        y = np.rint(2.0 * rng.standard_normal(n)) + rng.uniform(-0.5, 0.5, n)
        claims = (0, 1, 2, 3)
    elif regime == "wide":
        loc = 3.0 * rng.standard_normal(n)
        scale = np.exp(rng.uniform(np.log(0.02), np.log(30.0), n))
        y = loc + scale * rng.uniform(-3.0, 3.0, n)
        claims = (0, 1)
    elif regime == "flip":
        loc = rng.uniform(2.0, 12.0, n) * np.where(rng.random(n) < 0.5, -1.0, 1.0)
        scale = np.exp(rng.uniform(np.log(0.05), np.log(5.0), n))
        y = loc * rng.uniform(0.505, 0.995, n)              # loc/2 < |y| < |loc|: both interval edges in the upper tail
        return _laplace_clean(y, loc, scale, safe=(3.0, 4.0, 1.0)) + ((0, 1, 2, 3),)
    elif regime == "tail":
        # far from loc on the side where both edges end in the LOWER tail (y beyond loc and loc/2: the flip reflects them
        # there; y below both: they are there already): no cancellation, float32 is accurate down to the floor, so a wrong
        # floor shows here where the three regimes above drown it in their own float32 error
        loc = 0.7 * rng.standard_normal(n)
        scale = np.exp(rng.uniform(np.log(0.05), np.log(2.0), n))
        d = 0.75 + scale * rng.uniform(0.0, 20.0, n)
        up = rng.random(n) < 0.5
        y = np.where(up, np.maximum(loc, 0.5 * loc) + d, np.minimum(loc, 0.5 * loc) - d)
        claims = (0, 1, 2, 3)
    else:
        raise ValueError(regime)
    return _laplace_clean(y, loc, scale) + (claims,)


def engineered_laplace_zero():
    """Elements whose three gradients are exactly 0: 2v == loc (sign 0), p == 0 far in either tail, scale at its floor."""
    y = [1.5, -2.0, 0.0, 100.25, -100.25, 7.0, 3.3, -4.7, 2.6]
    loc = [3.0, -4.0, 0.0, 0.0, 0.0, -3.0, 0.1, 0.2, 7.0]
    scale = [1.0, 0.3, 1e-9, 0.5, 0.5, 0.05, 1e-9, 1e-9, 1e-9]
    return _f32(y), _f32(loc), _f32(scale)


def engineered_laplace_edge():
    """scale at its floor with y + 0.5 == loc exactly: one CDF edge sits on the peak of a density of height 5e8."""
    y = [0.0, 2.5, -3.5, 5.25]
    loc = [0.5, 3.0, -3.0, 5.75]
    return _f32(y), _f32(loc), np.full(4, 1e-9, np.float32)


def engineered_laplace_edge_wide():
    """The same tie at ordinary scales, where the other edge still has its density: the edge on loc adds none (gradient of
    tf.abs: sign(0) = 0), in float32 and float64 alike.  Such ties do occur in a training step: y~ - 0.5 rounds onto loc."""
    y = [0.0, 2.5, -3.5, 5.25, 1.0, -2.25]
    loc = [0.5, 3.0, -3.0, 5.75, 0.5, -2.75]            # the last two: y - 0.5 == loc
    return _f32(y), _f32(loc), _f32([1.0, 0.7, 2.0, 0.3, 1.0, 0.6])


# ------------------------------------------------------------------ factorized prior
def pack_params(w):
    """The kernels' packed parameter vector: the twelve estimator tensors in EB_NAMES order, each raveled."""
    return np.concatenate([_f32(w["estimator/" + n]).ravel() for n in EB_NAMES])


def unpack_params(vec, C):
    """Inverse of pack_params (also unpacks dparams) -> dict name -> [C, rows, cols]."""
    f = (1, 3, 3, 3, 1)
    out, off = {}, 0
    for n in EB_NAMES:
        i = int(n[-1])
        shape = (C, f[i + 1], f[i]) if n.startswith("matrix") else (C, f[i + 1], 1)
        k = int(np.prod(shape))
        out["estimator/" + n] = np.asarray(vec[off:off + k]).reshape(shape)
        off += k
    assert off == len(vec) == 44 * C
    return out


def factorized_grad(z, w, coef, dtype=torch.float64, bound=BOUND):
    """z: n floats, element i of channel i % C (the kernels' [m, C] layout).  Gradients of coef * sum(log(max(p, bound))),
    p = oracle.train._eb_likelihood -> (dz [n], dparams packed [44 C], p [n])."""
    C = int(np.asarray(w["estimator/matrix_0"]).shape[0])
    z = _f32(z).reshape(-1, C)
    wt = {"estimator/" + n: _leaf(w["estimator/" + n], dtype) for n in EB_NAMES}
    c = float(np.float32(coef))
    step = max(1, _CHUNK // C)
    dz, ps = [], []
    for a in range(0, z.shape[0], step):
        zc = z[a:a + step]
        t = _leaf(zc.T.reshape(1, C, -1, 1, 1), dtype)
        p = otrain._eb_likelihood(wt, t)
        (c * torch.log(torch.clamp_min(p, bound)).sum()).backward()
        dz.append(t.grad.numpy().reshape(C, -1).T)
        ps.append(p.detach().numpy().reshape(C, -1).T)
    dparams = np.concatenate([wt["estimator/" + n].grad.numpy().ravel() for n in EB_NAMES])
    return np.concatenate(dz).ravel(), dparams, np.concatenate(ps).ravel()


def eb_weights(C, perturbed, seed=0):
    """Estimator tensors for C channels: synthetic.make_weights(profile="dense") for C = 8, rows of make_weights_simple
    (repeated above its 32) otherwise; perturbed adds 0.5 * N to every entry so that no two channels are alike (with
    identical channels a wrong channel index is invisible)."""
    from pcgcv1_amd import synthetic
    src = synthetic.make_weights(seed=5, profile="dense") if C == 8 else synthetic.make_weights_simple(seed=5)
    rng = np.random.default_rng(2000 + 7 * C + seed)
    w = {}
    for n in EB_NAMES:
        a = _f32(src["estimator/" + n])
        a = a[np.arange(C) % a.shape[0]].copy()
        if perturbed:
            a = a + (0.5 * rng.standard_normal(a.shape)).astype(np.float32)
        w["estimator/" + n] = _f32(a)
    return w


FZ_ENGINEERED = (60.0, -60.0, 1000.0, -1000.0)
FZ_CHANNELS = (1, 8, 16, 32, 64, 128, 256)
# (elements per channel, perturbed weights): raw weights only at the middle size, to keep the CPU reference quick
FZ_DRAWS_ONE = 16               # the m = 1 case is this many draws (seed = 0 ...), judged together
FZ_KINDS = (("one", True), ("trip", False), ("trip", True), ("4096", True))


def fz_m(C, kind):
    """elements per channel: 1 (nearly all of the 256 blocks write zero partials); n = 65 536 + 3 C (256 blocks of 256 threads
    cover 65 536 in one trip, 3 C threads take a second); 4096."""
    return {"one": 1, "trip": 65536 // C + 3, "4096": 4096}[kind]


def gen_factorized(C, m, w, seed=0):
    """-> z [m * C] float32 (alternating rows of 2 * N and 6 * N) with the engineered tail elements written over a few places
    when there is room, and the indices of those places.  +-60 is deep in the tail (p64 down to 1e-17 with the perturbed
    weights, but up to 6e-3 in the widest synthetic channels); +-1000 is below the floor in every channel of every weight set
    (p64 < 1e-16, checked by the host test)."""
    rng = np.random.default_rng(3000 + 13 * C + m + seed)
    z = rng.standard_normal((m, C)) * np.where(np.arange(m) % 2 == 0, 2.0, 6.0)[:, None]
    if m == 1:
        z = rng.standard_normal((m, C)) * np.where(np.arange(C) % 2 == 0, 2.0, 6.0)[None, :]
    z = _f32(z).ravel()
    eng = np.zeros(0, np.int64)
    if z.size >= 64:
        eng = (np.arange(16) * 977 + 5) % z.size
        z[eng] = np.resize(_f32(FZ_ENGINEERED), eng.size)
    p64 = factorized_grad(z, w, 1.0)[2]
    z[(p64 >= BOUND / 2) & (p64 <= 2 * BOUND)] = 0.0
    return z, eng


# ------------------------------------------------------------------ BCE
def bce_grad(pred, label, c0, c1, dtype=torch.float64):
    """d/dpred of c0 * sum_{label == 0} -log(1 - o) + c1 * sum_{label > 0} -log(o), o = clip(sigmoid(pred), 1e-7, 1 - 1e-7)
    (the BCE lines of oracle.train.forward_loss with the two means' 1/n folded into c0, c1) -> (dpred, o)."""
    pred, label = _f32(pred), _f32(label)
    c0, c1 = float(np.float32(c0)), float(np.float32(c1))
    g, os_ = [], []
    for a in range(0, pred.size, _CHUNK):
        x_t = _leaf(pred[a:a + _CHUNK], dtype)
        lab = torch.from_numpy(label[a:a + _CHUNK])
        occ = torch.clamp(torch.sigmoid(x_t), 1e-7, 1.0 - 1e-7)
        empty = (-torch.log(1.0 - occ))[lab == 0].sum()
        full = (-torch.log(occ))[lab > 0].sum()
        (c0 * empty + c1 * full).backward()
        g.append(x_t.grad.numpy())
        os_.append(occ.detach().numpy())
    return np.concatenate(g), np.concatenate(os_)


BCE_LABELS = (0.0, 1.0, 0.5, 2.0, -1.0)       # 0.5 and 2 count as occupied, -1 belongs to neither class
_PRED_MAX = float(np.log(1.0 / (2 * CLIP) - 1.0))        # sigmoid(-x) = 2e-7: a factor 2 inside the clip (15.42)


def margin_bce(pred):
    return np.abs(np.asarray(pred, np.float64)) <= _PRED_MAX


def gen_bce(n=N_BIG, seed=0):
    rng = np.random.default_rng(4000 + seed)
    pred = _f32(rng.uniform(-16.0, 16.0, n))
    pred[~margin_bce(pred)] = 0.125
    label = _f32(BCE_LABELS)[rng.choice(5, n, p=(0.4, 0.25, 0.1, 0.1, 0.15))]
    return pred, label


def bce_factor(pred, label):
    """float64 factor of the gradient the bins go by: o for an empty voxel, 1 - o for an occupied one, nan for neither."""
    x = np.asarray(pred, np.float64)
    o = 1.0 / (1.0 + np.exp(-x))
    one_minus = 1.0 / (1.0 + np.exp(x))
    return np.where(label == 0, o, np.where(label > 0, one_minus, np.nan))


def engineered_bce():
    """-> (pred, label, inside): |pred| >= 17 is outside the clip in float32 and float64 alike (exactly 0); +-16.0 is inside
    in both (sigmoid(-16) = 1.125e-7 >= 1e-7; float32 rounds 1 - 1.125e-7 to 1 - 2^-23, its own 1 - 1e-7)."""
    pred = _f32([17.0, -17.0, 17.0, -17.0, 30.0, -30.0, 88.0, -104.0, 16.0, -16.0, 16.0, -16.0, 16.0, 3.0])
    label = _f32([0.0, 0.0, 1.0, 1.0, 0.0, 2.0, 1.0, 0.0, 0.0, 0.0, 1.0, 1.0, -1.0, -1.0])
    inside = np.abs(pred) <= 16.0
    return pred, label, inside


# ------------------------------------------------------------------ pure selections (TensorFlow tie conventions)
def abs_max_fwd(s, lb):
    return np.maximum(np.abs(_f32(s)), np.float32(lb))


def abs_max_bwd(dscale, s, lb):
    """where(|s| >= lb, dscale * sign(s), 0): tf.maximum sends the whole gradient to its first argument on a tie."""
    s, dscale = _f32(s), _f32(dscale)
    sg = np.where(s > 0, np.float32(1), np.where(s < 0, np.float32(-1), np.float32(0))).astype(np.float32)
    return np.where(np.abs(s) >= np.float32(lb), dscale * sg, np.float32(0)).astype(np.float32)


def margin_abs_max(s, lb):
    a = np.abs(np.asarray(s, np.float64))
    return (a < lb / 2) | (a > 2 * lb)


def gen_abs_max(lb, n, seed=0):
    """-> (s, dscale, n_engineered): random s clear of lb by a factor 2, then +-0, |s| == lb with both signs and |s| one ulp
    either side of lb written over the first places."""
    rng = np.random.default_rng(5000 + seed)
    s = _f32(rng.standard_normal(n) * (0.2 if lb > 1e-3 else 1.0))
    if lb <= 1e-3:
        s[rng.random(n) < 0.3] *= np.float32(1e-10)            # below the trainer's 1e-9 as often as above
    s[~margin_abs_max(s, lb)] = np.float32(4 * lb)
    l32 = np.float32(lb)
    up, dn = np.nextafter(l32, np.float32(1)), np.nextafter(l32, np.float32(0))
    eng = _f32([0.0, -0.0, l32, -l32, up, -up, dn, -dn])
    k = min(n, eng.size)
    s[:k] = eng[:k]
    return s, _f32(rng.standard_normal(n)), k


def relu_bwd(dy, dy_cs, dy_co, y, nvox, C):
    g = _f32(dy).reshape(nvox, dy_cs)[:, dy_co:dy_co + C]
    return _f32(g if y is None else np.where(_f32(y).reshape(nvox, C) > 0, g, np.float32(0))).ravel()


def gen_relu(nvox, C, dy_cs, seed=0):
    """-> (dy [nvox * dy_cs], y [nvox * C]) with 0.0, -0.0 and denormals of both signs spread through y."""
    rng = np.random.default_rng(6000 + seed)
    dy = _f32(rng.standard_normal(nvox * dy_cs))
    y = _f32(rng.standard_normal(nvox * C))
    special = _f32([0.0, -0.0, 1e-40, -1e-40, 1.4e-45, -1.4e-45])
    idx = np.arange(0, y.size, 3)
    y[idx] = special[np.arange(idx.size) % special.size]
    return dy, y
