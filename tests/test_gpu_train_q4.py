"""-m gpu: the kernels Trainer(q4=True) — the default — runs on the Q4 layout [b][d][h][C/4][w][4] of the 64^3 stage, one by one:
the three fused block kernels against their NDHWC twins bit for bit, every weight gradient that reads a Q4 operand against the
same kernel on NDHWC tensors bit for bit (and one of them against a float64 reference), the four boundary layers conv_in /
down_1 / up_2 / deconv_out forward and bwd-data against the NDHWC layer (bit for bit where both run the implicit-GEMM kernels)
and against a float64 reference on the host (the inference path's row kernels sum in another order), and the refusals of shapes
without a Q4 kernel.  The whole-step comparison of the two layouts (test_gpu_train.py) allows 2e-4 ... 6e-4 of a parameter's
largest gradient; one wrong cube face, channel quad or mask layout fits under that and not under these."""
import contextlib
import ctypes

import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from oracle import train as otrain                      # noqa: E402
from pcgcv1_amd import _lib                               # noqa: E402
from pcgcv1_amd.models import spec                        # noqa: E402
from pcgcv1_amd.train_hyper import Trainer, _TrainLayer   # noqa: E402  (no Trainer is created: its layout table and the plan's struct)

P = _lib.dptr


def _to_q4(x):
    """NDHWC -> Q4, the formula of the header; the result keeps the nominal shape [B,D,D,D,C] (as the Trainer's tensors do)."""
    B, D, C = x.shape[0], x.shape[1], x.shape[-1]
    return x.view(B, D, D, D, C // 4, 4).permute(0, 1, 2, 4, 3, 5).contiguous().view(B, D, D, D, C)


def _from_q4(y):
    B, D, C = y.shape[0], y.shape[1], y.shape[-1]
    return y.view(B, D, D, C // 4, D, 4).permute(0, 1, 2, 4, 3, 5).contiguous().view(B, D, D, D, C)


def _refused(rc, needle):
    """A refusal: non-zero return and a message that names what was refused."""
    err = _lib.hip().pcgc_last_error()
    return rc != 0 and len(err) > 0 and needle in err


# ------------------------------------------------------------------ 0. the layout helper
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("D", [32, 64])
@pytest.mark.parametrize("C", [8, 16])
def test_layout_q4_is_the_permutation_of_the_header(C, D, B):
    """pcgc_layout_q4 against x.view(B,D,D,D,C//4,4).permute(0,1,2,4,3,5) in both directions, on arange (every element
    distinct: at most 3 * 64^3 * 16 < 2^24 values, all exact in float32), so any permutation error shows."""
    lib, dev = _lib.hip(), _lib.require_gpu()
    n = B * D ** 3 * C
    assert n < 1 << 24
    x = torch.arange(n, dtype=torch.float32, device=dev).view(B, D, D, D, C)
    q, back = torch.full_like(x, -1.0), torch.full_like(x, -1.0)
    _lib.check(lib.pcgc_layout_q4(P(x), P(q), B, D, C, 1, _lib.stream()), "pcgc_layout_q4")
    assert torch.equal(q, _to_q4(x))
    assert torch.equal(q.view(B, D, D, C // 4, D, 4)[1 % B, 3, 5, 1, 7], x[1 % B, 3, 5, 7, 4:8])    # the formula itself, one quad spelled out
    _lib.check(lib.pcgc_layout_q4(P(q), P(back), B, D, C, 0, _lib.stream()), "pcgc_layout_q4")
    assert torch.equal(back, x) and torch.equal(_from_q4(q), x)


# ------------------------------------------------------------------ 1. the block kernels against their NDHWC twins
_D, _C, _Q, _H = 64, 16, 4, 8


def _block_params(g, dev):
    """conv1_1, conv1_2, conv2_1, conv2_2, conv2_3 (kernel, bias each) of a C = 16 block, every tap and channel pair distinct."""
    C, Q, H = _C, _Q, _H
    shapes = [(3, 3, 3, C, Q), (Q,), (3, 3, 3, Q, H), (H,), (1, 1, 1, C, Q), (Q,), (3, 3, 3, Q, Q), (Q,), (1, 1, 1, Q, H), (H,)]
    return [(torch.randn(sh, generator=g) * (0.15 if len(sh) > 1 else 0.05)).to(dev) for sh in shapes]


@pytest.mark.parametrize("B", [1, 3])
def test_vrn_fwd_train_q4_equals_the_ndhwc_kernel(B):
    """pcgc_vrn_fwd_train_q4 against pcgc_vrn_fwd_train_signs on the same block: t11 / t21 / t22 (4 channels: the same in both
    layouts) and all 28 bits of the sign words identical, `out` identical after converting back; a second call gives the same
    bits.  The same sums from other addresses, so nothing but torch.equal."""
    lib, dev = _lib.hip(), _lib.require_gpu()
    g = torch.Generator(device="cpu").manual_seed(131 + B)
    D, C, Q = _D, _C, _Q
    params = _block_params(g, dev)
    arr = ctypes.cast((ctypes.c_void_p * 10)(*[p.data_ptr() for p in params]), ctypes.c_void_p)
    x = torch.relu(torch.randn((B, D, D, D, C), generator=g)).to(dev)
    xq = torch.empty_like(x)
    _lib.check(lib.pcgc_layout_q4(P(x), P(xq), B, D, C, 1, _lib.stream()), "pcgc_layout_q4")

    def outputs():
        return [torch.full((B, D, D, D, Q), 7.0, device=dev) for _ in range(3)] + \
               [torch.full((B, D, D, D), -1, dtype=torch.int32, device=dev), torch.full_like(x, 7.0)]
    a, b, b2 = outputs(), outputs(), outputs()
    _lib.check(lib.pcgc_vrn_fwd_train_signs(P(x), arr, *[P(t) for t in a], B, D, C, _lib.stream()), "pcgc_vrn_fwd_train_signs")
    _lib.check(lib.pcgc_vrn_fwd_train_q4(P(xq), arr, *[P(t) for t in b], B, D, C, _lib.stream()), "pcgc_vrn_fwd_train_q4")
    _lib.check(lib.pcgc_vrn_fwd_train_q4(P(xq), arr, *[P(t) for t in b2], B, D, C, _lib.stream()), "pcgc_vrn_fwd_train_q4")
    for i, name in enumerate(("t11", "t21", "t22", "signs")):
        assert torch.equal(a[i], b[i]), name
        assert torch.equal(b[i], b2[i]), name + " (repeat)"
    assert int((a[3] >> 28).abs().max()) == 0 and 0.05 < float((a[3] & 1).float().mean()) < 0.95
    assert torch.equal(_from_q4(b[4]), a[4]), "out"
    assert torch.equal(b[4], b2[4]), "out (repeat)"
    assert float(a[4].abs().max()) > 0 and not torch.equal(b[4], a[4])          # Q4 really is another order of the same values


@pytest.mark.parametrize("B", [1, 3])
def test_vrn_bwd_tail_split_q4_equals_the_ndhwc_kernel(B):
    """pcgc_vrn_bwd_tail_split_q4 (dout, dz12, dz23 in Q4; dt11 / dt21 / dt22 plain) against pcgc_vrn_bwd_tail_split: all five
    outputs bit for bit, the sign words built as test_vrn_bwd_tail_split_equals_split_then_tail builds them (masks in bits
    16-27), outputs pre-filled with 7.0; a second call gives the same bits."""
    lib, dev = _lib.hip(), _lib.require_gpu()
    g = torch.Generator(device="cpu").manual_seed(143 + B)
    D, C, Q, H = _D, _C, _Q, _H
    dout = torch.randn((B, D, D, D, C), generator=g).to(dev)
    signs = torch.randint(0, 1 << 16, (B, D, D, D), generator=g, dtype=torch.int32).to(dev)
    t11, t21, t22 = (torch.randn((B, D, D, D, Q), generator=g).to(dev) for _ in range(3))
    for base, t in ((16, t22), (20, t11), (24, t21)):
        for i in range(4):
            signs |= (t[..., i] > 0).to(torch.int32) << (base + i)
    w12 = (torch.randn((3, 3, 3, Q, H), generator=g) * 0.1).to(dev)
    w22 = (torch.randn((3, 3, 3, Q, Q), generator=g) * 0.15).to(dev)
    w23 = (torch.randn((1, 1, 1, Q, H), generator=g) * 0.3).to(dev)
    doutq = _to_q4(dout)

    def outputs():
        return [torch.full((B, D, D, D, H), 7.0, device=dev) for _ in range(2)] + [torch.full((B, D, D, D, Q), 7.0, device=dev) for _ in range(3)]
    a, b, b2 = outputs(), outputs(), outputs()
    fixed = [P(signs), P(t11), P(t21), P(t22), P(w12), P(w22), P(w23)]
    _lib.check(lib.pcgc_vrn_bwd_tail_split(P(dout), *fixed, *[P(t) for t in a], B, D, C, _lib.stream()), "pcgc_vrn_bwd_tail_split")
    _lib.check(lib.pcgc_vrn_bwd_tail_split_q4(P(doutq), *fixed, *[P(t) for t in b], B, D, C, _lib.stream()), "pcgc_vrn_bwd_tail_split_q4")
    _lib.check(lib.pcgc_vrn_bwd_tail_split_q4(P(doutq), *fixed, *[P(t) for t in b2], B, D, C, _lib.stream()), "pcgc_vrn_bwd_tail_split_q4")
    for i, name in enumerate(("dz12", "dz23", "dt11", "dt21", "dt22")):
        got = _from_q4(b[i]) if i < 2 else b[i]
        assert torch.equal(got, a[i]), name
        assert torch.equal(b[i], b2[i]), name + " (repeat)"
        assert float(a[i].abs().max()) > 0 and not bool((a[i] == 7.0).any()), name


@pytest.mark.parametrize("mask", [True, False])
@pytest.mark.parametrize("B", [1, 3])
def test_vrn_bwd_input_q4_equals_the_ndhwc_kernel(B, mask):
    """pcgc_vrn_bwd_input_q4 (dpre, x_mask, dx in Q4) against pcgc_vrn_bwd_input, in place on dpre, with and without the mask of
    the block input: bit for bit, and again on a second call."""
    lib, dev = _lib.hip(), _lib.require_gpu()
    g = torch.Generator(device="cpu").manual_seed(157 + B)
    D, C, Q = _D, _C, _Q
    dt11, dt21 = (torch.randn((B, D, D, D, Q), generator=g).to(dev) for _ in range(2))
    dpre = torch.randn((B, D, D, D, C), generator=g).to(dev)
    x = torch.relu(torch.randn((B, D, D, D, C), generator=g)).to(dev)
    w11 = (torch.randn((3, 3, 3, C, Q), generator=g) * 0.1).to(dev)
    w21 = (torch.randn((1, 1, 1, C, Q), generator=g) * 0.3).to(dev)
    xq = _to_q4(x)
    a, b, b2 = dpre.clone(), _to_q4(dpre), _to_q4(dpre)
    _lib.check(lib.pcgc_vrn_bwd_input(P(dt11), P(dt21), P(a), P(x) if mask else None, P(w11), P(w21), P(a), B, D, C, _lib.stream()),
               "pcgc_vrn_bwd_input")
    for t in (b, b2):
        _lib.check(lib.pcgc_vrn_bwd_input_q4(P(dt11), P(dt21), P(t), P(xq) if mask else None, P(w11), P(w21), P(t), B, D, C, _lib.stream()),
                   "pcgc_vrn_bwd_input_q4")
    assert torch.equal(_from_q4(b), a)
    assert torch.equal(b, b2)
    assert not torch.equal(a, dpre)
    if mask:
        assert bool((a[x == 0] == 0).all()) and float((a == 0).float().mean()) < 0.55     # the mask's zeros, about half


# ------------------------------------------------------------------ plans that hold every layer twice: Q4 and NDHWC
def _stage_layers():
    """The layers of the 64^3 stage whose plan entries get a Q4 flag, from the model's own tables: name -> (net, Layer, D of
    the layer's input)."""
    an = {l.name: l for l in spec.analysis_layers()}
    sy = {l.name: l for l in spec.synthesis_layers()}
    return {"conv_in": ("analysis_transform", an["conv_in"], 64), "deconv_out": ("synthesis_transform", sy["deconv_out"], 64),
            "conv1_2": ("analysis_transform", an["vrn1_1/conv1_2"], 64), "conv2_3": ("analysis_transform", an["vrn1_1/conv2_3"], 64),
            "conv1_1": ("analysis_transform", an["vrn1_1/conv1_1"], 64), "conv2_1": ("analysis_transform", an["vrn1_1/conv2_1"], 64),
            "down_1": ("analysis_transform", an["down_1"], 64), "up_2": ("synthesis_transform", sy["up_2"], 32)}


_WANT_FLAGS = {"conv_in": (0, 1), "deconv_out": (1, 0), "conv1_2": (0, 1), "conv2_3": (0, 1), "conv1_1": (1, 0), "conv2_1": (1, 0),
               "down_1": (1, 0), "up_2": (0, 1)}


class _TwoCopyPlan(object):
    """One pcgc_train_plan with every named layer twice on the SAME filter: entry q[name] with the layout flags
    Trainer._q4_flags gives it (pcgc_train_plan_set_layout), entry n[name] left at (0, 0); gradients gk / gb per entry."""

    def __init__(self, names, kernels, dev):
        lib = _lib.hip()
        table = _stage_layers()
        self.names, self.dev = list(names), dev
        self.layer = {k: table[k][1] for k in names}
        self.D = {k: table[k][2] for k in names}
        self.flags = {k: Trainer._q4_flags(table[k][0], table[k][1]) for k in names}
        for k in names:
            assert self.flags[k] == _WANT_FLAGS[k], (k, self.flags[k])
        self.k = {k: kernels[k].to(dev).contiguous() for k in names}
        self.q = {k: i for i, k in enumerate(names)}
        self.n = {k: len(names) + i for i, k in enumerate(names)}
        self.gk, self.gb = {}, {}
        arr = (_TrainLayer * (2 * len(names)))()
        for k in names:
            l = self.layer[k]
            assert tuple(self.k[k].shape) == spec.kernel_shape(l), k
            for i in (self.q[k], self.n[k]):
                self.gk[i] = torch.full_like(self.k[k], 7.0)
                self.gb[i] = torch.full((l.cout,), 7.0, device=dev) if l.bias else None
                arr[i].kernel, arr[i].dkernel = self.k[k].data_ptr(), self.gk[i].data_ptr()
                arr[i].dbias = self.gb[i].data_ptr() if l.bias else None
                arr[i].Cin, arr[i].Cout, arr[i].ksize = l.cin, l.cout, l.k
                arr[i].stride, arr[i].transposed = (2, 1) if l.kind == "tconv" else (l.stride, 0)
        self.plan = ctypes.c_void_p()
        _lib.check(lib.pcgc_train_plan_create(ctypes.cast(arr, ctypes.c_void_p), 2 * len(names), ctypes.byref(self.plan)), "pcgc_train_plan_create")
        for k in names:
            _lib.check(lib.pcgc_train_plan_set_layout(self.plan, self.q[k], *self.flags[k]), "pcgc_train_plan_set_layout")
            _lib.check(lib.pcgc_train_plan_set_layout(self.plan, self.n[k], 0, 0), "pcgc_train_plan_set_layout")

    def out_shape(self, name, B):
        l, D = self.layer[name], self.D[name]
        Do = 2 * D if l.kind == "tconv" else D // l.stride
        return (B, Do, Do, Do, l.cout)

    def fwd(self, name, q4, x, bias, relu):
        """The layer's forward on x (NDHWC); q4: through the Q4 entry, operands converted on the way in and out."""
        B, (xq, yq) = int(x.shape[0]), self.flags[name]
        y = torch.full(self.out_shape(name, B), 7.0, device=self.dev)
        xin = _to_q4(x) if (q4 and xq) else x
        _lib.check(_lib.hip().pcgc_train_conv_fwd(self.plan, (self.q if q4 else self.n)[name], P(xin), P(bias), P(y), B, self.D[name], int(relu),
                                                  _lib.stream()), "pcgc_train_conv_fwd " + name)
        return _from_q4(y) if (q4 and yq) else y

    def bwd_data(self, name, q4, dz, mask, add_to=None):
        """dx of the layer (NDHWC in, NDHWC out); q4: through the Q4 entry (dz converted when y is Q4; mask, add_to and dx when x is)."""
        l, D, B, (xq, yq) = self.layer[name], self.D[name], int(dz.shape[0]), self.flags[name]
        conv_x = (lambda t: _to_q4(t) if (q4 and xq and t is not None) else t)
        dx = torch.full((B, D, D, D, l.cin), 7.0, device=self.dev)
        # (named, so that every converted operand stays allocated until the call has been queued)
        dz_in, mask_in, add_in = (_to_q4(dz) if (q4 and yq) else dz), conv_x(mask), conv_x(add_to)
        rc = _lib.hip().pcgc_train_conv_bwd_data(self.plan, (self.q if q4 else self.n)[name], P(dz_in), P(dx), P(mask_in), P(add_in), B, D,
                                                 _lib.stream())
        return rc, (_from_q4(dx) if (q4 and xq) else dx)

    def close(self):
        plan, self.plan = self.plan, None
        if plan:
            _lib.hip().pcgc_train_plan_destroy(plan)


@contextlib.contextmanager
def _two_copy_plan(names, kernels, dev):
    p = _TwoCopyPlan(names, kernels, dev)
    try:
        yield p
    finally:
        p.close()


def _kernels(g, names):
    table = _stage_layers()
    return {k: torch.randn(spec.kernel_shape(table[k][1]), generator=g) * 0.2 for k in names}


# ------------------------------------------------------------------ 2. weight gradients
@pytest.mark.parametrize("B", [1, 3])
def test_weight_gradients_on_q4_operands_equal_the_ndhwc_layers(B):
    """Every weight gradient of the step that reads a Q4 operand against the same layer on NDHWC tensors, through the plan
    (prepare, bwd_weight / bwd_weight_pair, finish_weights): conv_in (dz Q4), deconv_out (x Q4), conv1_2 and conv2_3 (dz Q4),
    conv1_1 | conv2_1 through pcgc_train_conv_bwd_weight_pair (x Q4), down_1 (x Q4, the fine operand) and up_2 (dz Q4, the fine
    operand, and the bias sums over a Q4 dz).  launch_conv_dw_tile / _s2 / _pair pick the same kernel for both layouts (edge,
    4xn<8>, 1x1<4,8>, 16xn<4,pair>, run_dw_mfma<32,2>) and the Q4 form only changes addresses: dkernel and dbias bit for bit
    (down_1 has no bias in the model, so none here).  conv1_2 also against a float64 sum over the 27 shifted views within the
    bound test_weight_gradient_pair_matches_the_single_calls uses, 2e-6 * max|ref| * sqrt(voxels summed), so that both layouts
    cannot be wrong together."""
    lib, dev = _lib.hip(), _lib.require_gpu()
    g = torch.Generator(device="cpu").manual_seed(211 + B)
    singles = ["conv_in", "deconv_out", "conv1_2", "conv2_3", "down_1", "up_2"]
    names = singles + ["conv1_1", "conv2_1"]
    st = _lib.stream()
    with _two_copy_plan(names, _kernels(g, names), dev) as tp:
        _lib.check(lib.pcgc_train_plan_prepare(tp.plan, st), "pcgc_train_plan_prepare")
        held = {}
        for name in singles:
            l, D, (xq, yq) = tp.layer[name], tp.D[name], tp.flags[name]
            x = torch.randn((B, D, D, D, l.cin), generator=g)
            x = (x if name == "conv_in" else torch.relu(x)).to(dev)             # every other layer reads a ReLU output
            dz = torch.randn(tp.out_shape(name, B), generator=g).to(dev)
            ops = (x, dz, _to_q4(x) if xq else x, _to_q4(dz) if yq else dz)
            held[name] = ops
            _lib.check(lib.pcgc_train_conv_bwd_weight(tp.plan, tp.q[name], P(ops[2]), P(ops[3]), B, D, st), "bwd_weight (Q4) " + name)
            _lib.check(lib.pcgc_train_conv_bwd_weight(tp.plan, tp.n[name], P(x), P(dz), B, D, st), "bwd_weight " + name)
        D = tp.D["conv1_1"]
        x = torch.relu(torch.randn((B, D, D, D, 16), generator=g)).to(dev)
        dz3, dz1 = (torch.randn((B, D, D, D, 4), generator=g).to(dev) for _ in range(2))
        xq4 = _to_q4(x)
        _lib.check(lib.pcgc_train_conv_bwd_weight_pair(tp.plan, tp.q["conv1_1"], tp.q["conv2_1"], P(xq4), P(dz3), P(dz1), B, D, st), "bwd_weight_pair (Q4)")
        _lib.check(lib.pcgc_train_conv_bwd_weight_pair(tp.plan, tp.n["conv1_1"], tp.n["conv2_1"], P(x), P(dz3), P(dz1), B, D, st), "bwd_weight_pair")
        _lib.check(lib.pcgc_train_plan_finish_weights(tp.plan, st), "pcgc_train_plan_finish_weights")
        for name in names:
            q, n = tp.q[name], tp.n[name]
            assert float(tp.gk[n].abs().max()) > 0 and not bool((tp.gk[n] == 7.0).any()), name
            assert torch.equal(tp.gk[q], tp.gk[n]), name + " dkernel"
            if tp.layer[name].bias:
                assert not bool((tp.gb[n] == 7.0).any()), name
                assert torch.equal(tp.gb[q], tp.gb[n]), name + " dbias"
            else:
                assert name == "down_1"
        # conv1_2 (4 -> 8, 3^3, 'same'): dk[kd,kh,kw] = sum_v x[v + k - 1] (x) dz[v], in double on the device
        x, dz = held["conv1_2"][0].double(), held["conv1_2"][1].double()
        D = tp.D["conv1_2"]
        xp = torch.nn.functional.pad(x, (0, 0, 1, 1, 1, 1, 1, 1))
        ref = torch.stack([torch.einsum("bdhwi,bdhwo->io", xp[:, kd:kd + D, kh:kh + D, kw:kw + D], dz)
                           for kd in range(3) for kh in range(3) for kw in range(3)]).view(3, 3, 3, 4, 8)
        ref_b = dz.sum((0, 1, 2, 3))
        nvox = B * D ** 3
        for i in (tp.q["conv1_2"], tp.n["conv1_2"]):
            err, tol = float((tp.gk[i].double() - ref).abs().max()), 2e-6 * float(ref.abs().max()) * nvox ** 0.5
            err_b, tol_b = float((tp.gb[i].double() - ref_b).abs().max()), 2e-6 * float(ref_b.abs().max()) * nvox ** 0.5
            print("conv1_2 B=%d %s: dkernel max err %.3g (bound %.3g), dbias max err %.3g (bound %.3g)" % (
                B, "Q4" if i == tp.q["conv1_2"] else "NDHWC", err, tol, err_b, tol_b))
            assert err <= tol and err_b <= tol_b, (i, err, tol, err_b, tol_b)


# ------------------------------------------------------------------ 3. the boundary layers, forward and bwd-data
_BOUNDARY = ["conv_in", "deconv_out", "down_1", "up_2"]
_RELU = {"conv_in": 1, "deconv_out": 0, "down_1": 1, "up_2": 1}
_B3 = 2


@pytest.fixture(scope="module")
def boundary():
    """Inputs of the four boundary layers at B = 2 (host tensors) and their float64 references, computed once and left unchanged:
    forward = relu(conv(x) + bias) with the padding of oracle/train.py::_conv (deconv_out: no ReLU); bwd-data = that convolution's
    adjoint applied to dz (torch autograd of the same call, in double)."""
    torch.set_num_threads(min(16, torch.get_num_threads()))
    g = torch.Generator(device="cpu").manual_seed(307)
    table = _stage_layers()
    kernels = _kernels(g, _BOUNDARY)
    nc, nl = (lambda t: t.permute(0, 4, 1, 2, 3)), (lambda t: t.permute(0, 2, 3, 4, 1).contiguous())
    data = {"kernels": kernels}
    for name in _BOUNDARY:
        _, l, D = table[name]
        Do = 2 * D if l.kind == "tconv" else D // l.stride
        x = torch.randn((_B3, D, D, D, l.cin), generator=g)
        x = x if name == "conv_in" else torch.relu(x)
        bias = torch.randn(l.cout, generator=g) * 0.1 if l.bias else None
        dz = torch.randn((_B3, Do, Do, Do, l.cout), generator=g)
        add_to = torch.randn((_B3, D, D, D, l.cin), generator=g)
        w = {"l/kernel": kernels[name].double()}
        xt = nc(x.double()).contiguous().requires_grad_(True)
        pre = otrain._conv(w, "l", xt, stride=l.stride, tconv=l.kind == "tconv")
        adj = None
        if name != "conv_in":                                                   # conv_in reads the occupancy grid: no gradient flows there
            (adj,) = torch.autograd.grad(pre, xt, nc(dz.double()).contiguous())
        pre = pre.detach() if bias is None else pre.detach() + bias.double().view(1, -1, 1, 1, 1)
        data[name] = {"x": x, "bias": bias, "dz": dz, "add_to": add_to, "fwd": nl(torch.relu(pre) if _RELU[name] else pre), "adj": nl(adj) if adj is not None else None}
    return data


def _on_device(entry, dev):
    return {k: (entry[k].to(dev) if entry[k] is not None else None) for k in ("x", "bias", "dz", "add_to")}


def _bound(ref):
    return 2e-5 * max(1.0, float(ref.abs().max()))


def test_resamplers_on_the_implicit_gemm_kernels_equal_the_ndhwc_layers(boundary, monkeypatch):
    """PCGC_TRAIN_ROW_RESAMPLE=0 (read per call): up_2 and down_1 with Q4 flags run the implicit-GEMM kernels the NDHWC layers
    run, reading / writing the Q4 side through other addresses — forward (ReLU on) and bwd-data with and without the ReLU mask
    bit for bit after converting the layout."""
    dev = _lib.require_gpu()
    monkeypatch.setenv("PCGC_TRAIN_ROW_RESAMPLE", "0")
    names = ["down_1", "up_2"]
    with _two_copy_plan(names, boundary["kernels"], dev) as tp:
        _lib.check(_lib.hip().pcgc_train_plan_prepare(tp.plan, _lib.stream()), "pcgc_train_plan_prepare")
        for name in names:
            d = _on_device(boundary[name], dev)
            ya, yb = tp.fwd(name, True, d["x"], d["bias"], 1), tp.fwd(name, False, d["x"], d["bias"], 1)
            assert torch.equal(ya, yb) and float(yb.max()) > 0 and float(yb.min()) == 0, name + " fwd"
            for mask in (d["x"], None):
                (ra, da), (rb, db) = tp.bwd_data(name, True, d["dz"], mask), tp.bwd_data(name, False, d["dz"], mask)
                assert ra == 0 and rb == 0, (name, _lib.hip().pcgc_last_error())
                assert torch.equal(da, db) and not bool((db == 7.0).any()), (name, mask is None)
                if mask is not None:
                    assert bool((db[mask == 0] == 0).all()) and float((db == 0).float().mean()) < 0.55, name


@pytest.mark.parametrize("name", _BOUNDARY)
def test_boundary_layers_match_a_float64_reference_in_both_layouts(boundary, name):
    """Default settings: with Q4 flags conv_in / deconv_out / up_2 / down_1 run the inference path's row kernels (another
    summation order; the ReLU mask of bwd-data applied in the store), forward and bwd-data: against the float64 reference of the
    fixture, max|got - ref| <= 2e-5 * max(1, max|ref|) — the bound test_vrn_bwd_input_matches_conv_transpose holds such sums to —
    with the NDHWC layer held to the same bound next to it, so a failure says which layout is wrong.  The mask is (x > 0) of the
    float32 tensor the kernel is given; every element is compared.  The bound is the project's, not a measurement; each case
    prints its largest error next to it (on an MI355X: 1.3e-6 ... 1.9e-5 against bounds of 1.1e-4 ... 4.2e-4, in both
    layouts)."""
    dev = _lib.require_gpu()
    d = _on_device(boundary[name], dev)
    with _two_copy_plan([name], boundary["kernels"], dev) as tp:
        _lib.check(_lib.hip().pcgc_train_plan_prepare(tp.plan, _lib.stream()), "pcgc_train_plan_prepare")
        results = []
        ref = boundary[name]["fwd"]
        for q4 in (True, False):
            got = tp.fwd(name, q4, d["x"], d["bias"], _RELU[name]).cpu().double()
            results.append(("fwd", q4, float((got - ref).abs().max()), _bound(ref)))
        if name != "conv_in":                                                   # conv_in's input is the occupancy grid: no gradient
            keep = (boundary[name]["x"] > 0).double()
            for mask, ref in ((d["x"], boundary[name]["adj"] * keep), (None, boundary[name]["adj"])):
                for q4 in (True, False):
                    rc, got = tp.bwd_data(name, q4, d["dz"], mask)
                    assert rc == 0, (name, q4, _lib.hip().pcgc_last_error())
                    results.append(("bwd-data mask" if mask is not None else "bwd-data", q4, float((got.cpu().double() - ref).abs().max()), _bound(ref)))
        for what, q4, err, tol in results:
            print("%s %s %s: max err %.3g (bound %.3g)" % (name, what, "Q4" if q4 else "NDHWC", err, tol))
        for what, q4, err, tol in results:
            assert err <= tol, (name, what, "Q4" if q4 else "NDHWC", err, tol)


@pytest.mark.parametrize("name", ["down_1", "up_2"])
def test_bwd_data_with_add_to_on_a_q4_resampler(boundary, name):
    """add_to bypasses the row kernels: down_1 / up_2 with Q4 flags then take the implicit-GEMM kernel, whose epilogue reads mask
    and add_to in the layout of dx.  dx = (mask > 0) * (add_to + conv^T(dz)) must equal the NDHWC layer's after conversion
    within 2e-5 * max(1, max|ref|) (and the float64 reference within the same bound), add_to apart from dx and aliasing it."""
    dev = _lib.require_gpu()
    d = _on_device(boundary[name], dev)
    ref = (boundary[name]["adj"] + boundary[name]["add_to"].double()) * (boundary[name]["x"] > 0).double()
    with _two_copy_plan([name], boundary["kernels"], dev) as tp:
        _lib.check(_lib.hip().pcgc_train_plan_prepare(tp.plan, _lib.stream()), "pcgc_train_plan_prepare")
        (ra, da), (rb, db) = tp.bwd_data(name, True, d["dz"], d["x"], d["add_to"]), tp.bwd_data(name, False, d["dz"], d["x"], d["add_to"])
        assert ra == 0 and rb == 0, (name, ra, rb, _lib.hip().pcgc_last_error())
        errs = (float((da - db).abs().max()), float((da.cpu().double() - ref).abs().max()), float((db.cpu().double() - ref).abs().max()))
        print("%s bwd-data add_to: Q4 - NDHWC %.3g, Q4 - ref %.3g, NDHWC - ref %.3g (bound %.3g)" % ((name,) + errs + (_bound(ref),)))
        assert max(errs) <= _bound(ref), (name, errs)
        # in place, as the step accumulates a gradient: add_to == dx, both Q4 on the flagged entry
        D, (xq, yq) = tp.D[name], tp.flags[name]
        acc = _to_q4(d["add_to"]) if xq else d["add_to"].clone()
        dz_in, mask_in = (_to_q4(d["dz"]) if yq else d["dz"]), (_to_q4(d["x"]) if xq else d["x"])
        _lib.check(_lib.hip().pcgc_train_conv_bwd_data(tp.plan, tp.q[name], P(dz_in), P(acc), P(mask_in), P(acc), _B3, D, _lib.stream()),
                   "bwd_data in place")
        assert torch.equal(_from_q4(acc) if xq else acc, da)


# ------------------------------------------------------------------ 4. refusals
def test_shapes_without_a_q4_kernel_are_refused_and_write_nothing():
    """include/pcgc.h: shapes without a kernel for Q4 tensors "fail with an error, never silently".  A 16 -> 16 3^3 layer flagged
    x_q4: forward, bwd-data and bwd-weight each return non-zero with a message about Q4 and leave their output (pre-filled with
    7.0) alone; the block entry points at D = 32, C = 32 likewise, naming themselves.  Host-side argument checks: nothing is
    launched."""
    lib, dev = _lib.hip(), _lib.require_gpu()
    g = torch.Generator(device="cpu").manual_seed(401)
    B, D, C = 1, 64, 16
    k = (torch.randn((3, 3, 3, C, C), generator=g) * 0.1).to(dev)
    gk, gb = torch.full_like(k, 7.0), torch.full((C,), 7.0, device=dev)
    arr = (_TrainLayer * 1)()
    arr[0].kernel, arr[0].dkernel, arr[0].dbias = k.data_ptr(), gk.data_ptr(), gb.data_ptr()
    arr[0].Cin, arr[0].Cout, arr[0].ksize, arr[0].stride, arr[0].transposed = C, C, 3, 1, 0
    plan = ctypes.c_void_p()
    _lib.check(lib.pcgc_train_plan_create(ctypes.cast(arr, ctypes.c_void_p), 1, ctypes.byref(plan)), "pcgc_train_plan_create")
    st = _lib.stream()
    try:
        _lib.check(lib.pcgc_train_plan_set_layout(plan, 0, 1, 0), "pcgc_train_plan_set_layout")
        _lib.check(lib.pcgc_train_plan_prepare(plan, st), "pcgc_train_plan_prepare")
        x = torch.relu(torch.randn((B, D, D, D, C), generator=g)).to(dev)
        dz = torch.randn((B, D, D, D, C), generator=g).to(dev)
        bias = torch.zeros(C, device=dev)
        y, dx = torch.full_like(x, 7.0), torch.full_like(x, 7.0)
        assert _refused(lib.pcgc_train_conv_fwd(plan, 0, P(x), P(bias), P(y), B, D, 1, st), b"Q4")
        assert _refused(lib.pcgc_train_conv_bwd_data(plan, 0, P(dz), P(dx), P(x), None, B, D, st), b"Q4")
        assert _refused(lib.pcgc_train_conv_bwd_weight(plan, 0, P(x), P(dz), B, D, st), b"Q4")
        _lib.check(lib.pcgc_train_plan_finish_weights(plan, st), "pcgc_train_plan_finish_weights")     # nothing was queued for it
        torch.cuda.synchronize()
        for t, name in ((y, "y"), (dx, "dx"), (gk, "dkernel"), (gb, "dbias")):
            assert bool((t == 7.0).all()), name
        # the same entry without the flag is an ordinary layer (the refusals above are about the layout, not the shape)
        _lib.check(lib.pcgc_train_plan_set_layout(plan, 0, 0, 0), "pcgc_train_plan_set_layout")
        _lib.check(lib.pcgc_train_conv_fwd(plan, 0, P(x), P(bias), P(y), B, D, 1, st), "pcgc_train_conv_fwd")
        assert not bool((y == 7.0).any())
        assert _refused(lib.pcgc_train_plan_set_layout(plan, 1, 1, 0), b"pcgc_train_plan_set_layout")
    finally:
        lib.pcgc_train_plan_destroy(plan)
    # the block entry points: Q4 kernels exist for D = 64 with C = 16 only
    D, C, Q, H = 32, 32, 8, 16
    shapes = [(3, 3, 3, C, Q), (Q,), (3, 3, 3, Q, H), (H,), (1, 1, 1, C, Q), (Q,), (3, 3, 3, Q, Q), (Q,), (1, 1, 1, Q, H), (H,)]
    params = [(torch.randn(sh, generator=g) * 0.1).to(dev) for sh in shapes]
    arr = ctypes.cast((ctypes.c_void_p * 10)(*[p.data_ptr() for p in params]), ctypes.c_void_p)
    x = torch.relu(torch.randn((B, D, D, D, C), generator=g)).to(dev)
    quarter = [torch.full((B, D, D, D, Q), 7.0, device=dev) for _ in range(3)]
    halves = [torch.full((B, D, D, D, H), 7.0, device=dev) for _ in range(2)]
    signs, out = torch.full((B, D, D, D), 7, dtype=torch.int32, device=dev), torch.full_like(x, 7.0)
    assert _refused(lib.pcgc_vrn_fwd_train_q4(P(x), arr, *[P(t) for t in quarter], P(signs), P(out), B, D, C, st), b"pcgc_vrn_fwd_train_q4")
    t = [torch.randn((B, D, D, D, Q), generator=g).to(dev) for _ in range(3)]
    assert _refused(lib.pcgc_vrn_bwd_tail_split_q4(P(x), P(signs), *[P(u) for u in t], P(params[2]), P(params[6]), P(params[8]),
                                                   *[P(u) for u in halves], *[P(u) for u in quarter], B, D, C, st), b"pcgc_vrn_bwd_tail_split_q4")
    dpre = torch.full_like(x, 7.0)
    assert _refused(lib.pcgc_vrn_bwd_input_q4(P(t[0]), P(t[1]), P(dpre), P(x), P(params[0]), P(params[4]), P(dpre), B, D, C, st), b"pcgc_vrn_bwd_input_q4")
    torch.cuda.synchronize()
    for u in quarter + halves + [out, dpre]:
        assert bool((u == 7.0).all())
    assert bool((signs == 7).all())
