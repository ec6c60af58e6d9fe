"""Float64 references and operands for the training step's kernels at batch sizes above the default — plain torch (pad, shifted
views, matmul in double, on whichever device the operands live on), no code of the package and no convolution routine of torch:
tests/test_train_batch_ref_host.py pins them to oracle.nets.vrn_block and to float64 autograd of oracle/train.py:_conv.

  block (C = 32 here; any C that is a multiple of 4), x NDHWC, filters in TensorFlow's layouts:
      t11 = relu(conv1_1(x))   3^3  C   -> C/4        t21 = relu(conv2_1(x))    1^3  C   -> C/4
      t12 = relu(conv1_2(t11)) 3^3  C/4 -> C/2        t22 = relu(conv2_2(t21))  3^3  C/4 -> C/4
                                                      t23 = relu(conv2_3(t22))  1^3  C/4 -> C/2
      pre = [t12 | t23],  out = relu(x + pre);  sign word of a voxel: bit c = (pre[c] > 0), as a 32-bit integer
  bwd-data of one layer:  dx = (mask > 0) * (add_to + conv^T(dz)), conv^T the adjoint of
      stride 1          y[o]  = sum_k x[o + k - (K - 1) // 2] W[k]          W [k,k,k,Cin,Cout]
      stride-2 conv     y[o]  = sum_k x[2 o + k - pb] W[k]                  pb = max(K - 2, 0) // 2 (TensorFlow's 'SAME')
      transposed conv   y[o]  = sum_{2 i + k - pb = o} x[i] W[k]^T          W [k,k,k,Cout,Cin]

Integer operands (tests/test_gpu_train_batch.py): x in {0, 1, 2} drawn like a ReLU output, filters in {-1, 0, 1}, biases in
{-2 .. 2}, add_to in {-3 .. 3}, dz in {-1, 0, 1}.  block_abs_bound / adjoint_abs_bound give, from those RANGES and the shapes
alone, the largest sum of |terms| any output can reach; below 2^24 every partial sum in any order is an integer float32 holds
exactly, so a kernel must EQUAL this reference whatever its summation order.
"""
import collections

import torch
import torch.nn.functional as F

EXACT = 2 ** 24
X_MAX, W_MAX, BIAS_MAX, ADD_MAX, DZ_MAX = 2, 1, 2, 3, 1        # the integer operands' ranges (largest magnitudes)

Block = collections.namedtuple("Block", "t11 t21 t22 pre out")


# ------------------------------------------------------------------ convolutions as sums of shifted matrix products
def conv_same(x, w, b=None):
    """stride 1, 'same': x [B,D,D,D,Ci], w [K,K,K,Ci,Co], b [Co] or None; float64 in, float64 out."""
    K, D = w.shape[0], x.shape[1]
    p = (K - 1) // 2
    xp = F.pad(x, (0, 0, p, p, p, p, p, p))
    y = torch.zeros(x.shape[:-1] + (w.shape[-1],), dtype=torch.float64, device=x.device)
    for kd in range(K):
        for kh in range(K):
            for kw in range(K):
                y += xp[:, kd:kd + D, kh:kh + D, kw:kw + D, :] @ w[kd, kh, kw]
    return y if b is None else y + b


def block_reference(x, params):
    """x [B,D,D,D,C]; params = [w11, b11, w12, b12, w21, b21, w22, b22, w23, b23] (the order of the block entry points) -> Block
    of float64 tensors."""
    x = x.double()
    w11, b11, w12, b12, w21, b21, w22, b22, w23, b23 = (p.double() for p in params)
    t11 = torch.relu(conv_same(x, w11, b11))
    t12 = torch.relu(conv_same(t11, w12, b12))
    t21 = torch.relu(conv_same(x, w21, b21))
    t22 = torch.relu(conv_same(t21, w22, b22))
    t23 = torch.relu(conv_same(t22, w23, b23))
    pre = torch.cat([t12, t23], dim=-1)
    return Block(t11, t21, t22, pre, torch.relu(x + pre))


def sign_words(pre):
    """bit c = (pre[..., c] > 0) for up to 32 channels, as the int32 the kernels store (bit 31 is the sign bit)."""
    C = pre.shape[-1]
    assert C <= 32
    weights = (2 ** torch.arange(C, dtype=torch.int64, device=pre.device))
    word = ((pre > 0).to(torch.int64) * weights).sum(-1)
    return torch.where(word >= 2 ** 31, word - 2 ** 32, word).to(torch.int32)


def conv_adjoint(dz, w, D, stride=1, transposed=False):
    """conv^T(dz) on the layer's input grid D^3: dz [B,Do,Do,Do,Cout] float64, w in the layer's TensorFlow layout -> [B,D,D,D,Cin]."""
    K, B, Do = w.shape[0], dz.shape[0], dz.shape[1]
    pb = max(K - 2, 0) // 2
    if transposed:                                     # dx[i] = sum_k dz[2 i + k - pb] W[k]   (W[k]: [Cout, Cin])
        assert Do == 2 * D
        dzp = F.pad(dz, (0, 0) + (pb, max(K - 2, 0) - pb) * 3)
        dx = torch.zeros((B, D, D, D, w.shape[4]), dtype=torch.float64, device=dz.device)
        span = 2 * (D - 1) + 1
        for kd in range(K):
            for kh in range(K):
                for kw in range(K):
                    dx += dzp[:, kd:kd + span:2, kh:kh + span:2, kw:kw + span:2, :] @ w[kd, kh, kw]
        return dx
    if stride == 2:                                    # dx[2 o + k - pb] += dz[o] W[k]^T
        assert 2 * Do == D
        buf = torch.zeros((B, D + K, D + K, D + K, w.shape[3]), dtype=torch.float64, device=dz.device)
        for kd in range(K):
            for kh in range(K):
                for kw in range(K):
                    buf[:, kd:kd + D:2, kh:kh + D:2, kw:kw + D:2, :] += dz @ w[kd, kh, kw].t()
        return buf[:, pb:pb + D, pb:pb + D, pb:pb + D, :].contiguous()
    assert stride == 1 and Do == D and K % 2 == 1      # dx[i] = sum_k dz[i - k + p] W[k]^T
    p = (K - 1) // 2
    dzp = F.pad(dz, (0, 0, p, p, p, p, p, p))
    dx = torch.zeros((B, D, D, D, w.shape[3]), dtype=torch.float64, device=dz.device)
    for kd in range(K):
        for kh in range(K):
            for kw in range(K):
                dx += dzp[:, K - 1 - kd:K - 1 - kd + D, K - 1 - kh:K - 1 - kh + D, K - 1 - kw:K - 1 - kw + D, :] @ w[kd, kh, kw].t()
    return dx


def bwd_data_reference(dz, w, D, stride=1, transposed=False, mask=None, add_to=None):
    """dx = (mask > 0) * (add_to + conv^T(dz)); mask is the float32 tensor the kernel is given (its sign is all that counts)."""
    dx = conv_adjoint(dz.double(), w.double(), D, stride, transposed)
    if add_to is not None:
        dx = dx + add_to.double()
    if mask is not None:
        dx = dx * (mask > 0).double()
    return dx


# ------------------------------------------------------------------ the exactness condition, from ranges and shapes alone
def block_abs_bound(C, x_max=X_MAX, w_max=W_MAX, b_max=BIAS_MAX):
    """Largest sum of |terms| of any output of the block (every layer's bias counted as a term, the residual sum included) when
    0 <= x <= x_max, |w| <= w_max, |b| <= b_max -> dict per tensor.  A ReLU output is at most the sum of |terms| behind it."""
    q = C // 4
    a11 = 27 * C * x_max * w_max + b_max
    a12 = 27 * q * a11 * w_max + b_max
    a21 = C * x_max * w_max + b_max
    a22 = 27 * q * a21 * w_max + b_max
    a23 = q * a22 * w_max + b_max
    return {"t11": a11, "t12": a12, "t21": a21, "t22": a22, "t23": a23, "out": x_max + max(a12, a23)}


def adjoint_abs_bound(cout, k, dz_max=DZ_MAX, w_max=W_MAX, add_max=ADD_MAX):
    """Largest sum of |terms| of a dx element: at most k^3 taps x Cout channels reach one input voxel (fewer in a strided
    layer), plus add_to."""
    return k ** 3 * cout * dz_max * w_max + add_max


# ------------------------------------------------------------------ operands (host generator: the same values on every machine)
def _gen(seed):
    return torch.Generator(device="cpu").manual_seed(seed)


def relu_like_ints(shape, g):
    """{0, 1, 2}: 0 three times in five, like the output of a ReLU (tests/test_gpu_train_dw.py)."""
    return torch.randint(-2, 3, shape, generator=g).clamp_(min=0).float()


def block_shapes(C):
    Q, H = C // 4, C // 2
    return [(3, 3, 3, C, Q), (Q,), (3, 3, 3, Q, H), (H,), (1, 1, 1, C, Q), (Q,), (3, 3, 3, Q, Q), (Q,), (1, 1, 1, Q, H), (H,)]


def set_faces(x):
    """The cube faces as tests/test_gpu_parity.py::test_vrn_block_vs_oracle sets them (rows / planes / lanes outside the cube
    must read as zeros: a constant face makes a wrong neighbour visible), in place."""
    x[:, 0], x[:, -1], x[:, :, 0], x[:, :, -1], x[:, :, :, 0], x[:, :, :, -1] = 1.5, -0.5, 2.0, 0.25, 1.0, 3.0
    return x


def set_faces_int(x):
    """The same for the integer operands: face values inside {0, 1, 2} (x stays a ReLU output)."""
    x[:, 0], x[:, -1], x[:, :, 0], x[:, :, -1], x[:, :, :, 0], x[:, :, :, -1] = 1.0, 0.0, 2.0, 1.0, 2.0, 1.0
    return x


def block_operands(kind, B, D, C, seed):
    """-> (x [B,D,D,D,C], params) float32 on the host; every cube its own values.  'int': the ranges of the header; 'gauss':
    x = relu(randn) with the faces of test_vrn_block_vs_oracle, filters He-scaled, biases 0.1 randn (as that test draws them)."""
    g = _gen(seed)
    if kind == "int":
        params = [torch.randint(-BIAS_MAX, BIAS_MAX + 1, sh, generator=g).float() if len(sh) == 1
                  else torch.randint(-W_MAX, W_MAX + 1, sh, generator=g).float() for sh in block_shapes(C)]
        return set_faces_int(relu_like_ints((B, D, D, D, C), g)), params
    params = [torch.randn(sh, generator=g) * (0.1 if len(sh) == 1 else (2.0 / (sh[0] ** 3 * sh[3])) ** 0.5) for sh in block_shapes(C)]
    return set_faces(torch.relu(torch.randn((B, D, D, D, C), generator=g))), params


def layer_shapes(cin, cout, k, stride, tr, D, B):
    """-> (dz shape, filter shape, x shape) of a layer given as (cin, cout, k, stride, transposed, D of its input)."""
    Do = 2 * D if tr else D // stride
    return (B, Do, Do, Do, cout), ((k, k, k, cout, cin) if tr else (k, k, k, cin, cout)), (B, D, D, D, cin)


def bwd_data_operands(kind, layer, B, seed):
    """-> dict(dz, w, mask, add_to) float32 on the host for layer = (cin, cout, k, stride, transposed, D)."""
    zs, ws, xs = layer_shapes(*layer, B)
    g = _gen(seed)
    if kind == "int":
        return {"dz": torch.randint(-DZ_MAX, DZ_MAX + 1, zs, generator=g).float(), "w": torch.randint(-W_MAX, W_MAX + 1, ws, generator=g).float(),
                "mask": relu_like_ints(xs, g), "add_to": torch.randint(-ADD_MAX, ADD_MAX + 1, xs, generator=g).float()}
    return {"dz": torch.randn(zs, generator=g), "w": torch.randn(ws, generator=g) * 0.2, "mask": torch.relu(torch.randn(xs, generator=g)),
            "add_to": torch.randn(xs, generator=g)}


# ------------------------------------------------------------------ the table of tests/test_gpu_train_batch.py
BLOCK_CASES = [(16, 32, 32), (17, 32, 32)]                     # (B, D, C): either side of launch_vrn32_row_train's B <= 16
BWD_LAYERS = [(64, 16, 3, 1, 0, 16), (16, 32, 3, 1, 0, 16), (64, 16, 1, 1, 0, 16), (16, 16, 3, 1, 0, 16), (16, 32, 1, 1, 0, 16),
              (32, 64, 3, 2, 0, 32), (64, 32, 3, 2, 1, 16)]    # (cin, cout, k, stride, transposed, D of the layer input)
# (layer, B): 19 | 20 cubes around B * (16/4)^2 * (16/16) < 320 at the 16^3 stage; 2 | 3 cubes around B * 8 * 8 * 2 < 320 at 32^3
BWD_CASES = [(l, B) for l in BWD_LAYERS for B in (19, 20)] + [((64, 16, 3, 1, 0, 32), 2), ((64, 16, 3, 1, 0, 32), 3)]
BWD_FORMS = ["plain", "mask", "add_to", "add_to aliasing dx", "mask + add_to"]


def bwd_case_id(case):
    (cin, cout, k, stride, tr, D), B = case
    return "%dto%d-k%d-%s-D%d-B%d" % (cin, cout, k, "tconv" if tr else "s%d" % stride, D, B)


def adjoint_grid(layer):
    """The grid edge launch_conv_mfma's `small` test uses for the layer's bwd-data: the coarse side of a strided layer."""
    cin, cout, k, stride, tr, D = layer
    return D // 2 if (stride == 2 and not tr) else D


def is_small_launch(layer, B):
    """csrc/conv_mfma.hip: small = B * (D/4) * (D/4) * (D/16) < 320 (fewer than 1.25 workgroups of 4 x 4 rows per compute unit)."""
    d = adjoint_grid(layer)
    return B * (d // 4) * (d // 4) * (d // 16) < 320
