"""Float64 reference for the filter and bias gradient of one convolution layer, in the repository's layouts — plain torch
(pad, strided views, matmul in double on whichever device the operands live on), no code of the package.

  stride 1          dk[kd, kh, kw, ci, co] = sum_o  x[o + k - (K - 1) // 2][ci] * dz[o][co]                o on the D^3 grid
  stride-2 conv     dk[kd, kh, kw, ci, co] = sum_o  x[2 o + k - pb][ci] * dz[o][co]                        o on the (D / 2)^3 grid
  transposed conv   dk[kd, kh, kw, co, ci] = sum_i  dz[2 i + k - pb][co] * x[i][ci]                        i on the D^3 grid
  bias              db[co] = sum of dz over all of its voxels

with pb = max(K - 2, 0) // 2, TensorFlow's 'SAME' front padding of a stride-2 layer (oracle/train.py:_conv), operands outside
their cube zero.  tests/test_dw_cases_host.py pins these conventions to float64 autograd of the oracle's convolution.

Next to every sum the reference returns S2 = the sum of the SQUARED terms over the same voxels, from which the tests derive
what float32 summation may cost (tests/test_gpu_train_dw.py).
"""
import collections

import torch
import torch.nn.functional as F

DwRef = collections.namedtuple("DwRef", "dk db s2k s2b n nb")
# dk, s2k: float64 in the layer's filter layout; db, s2b: float64 [Cout]; n, nb: voxels one filter / bias element sums over


def _tap_sums(fine, coarse, K, step, front, back):
    """out[kd, kh, kw, a, c] = sum over (b, o) of fine[b, step * o + k - front, a] * coarse[b, o, c] — and the same sum of the
    squared products; fine [B, F, F, F, Ca] and coarse [B, n, n, n, Cc] in float64."""
    n = coarse.shape[1]
    Ca, Cc = fine.shape[-1], coarse.shape[-1]
    fp = F.pad(fine, (0, 0, front, back, front, back, front, back))
    assert fp.shape[1] >= step * (n - 1) + K, (fp.shape, n, K, step)
    # one small matrix product per row of n voxels, then the sum over the rows: a single [Ca x voxels] @ [voxels x Cc] product
    # has one output tile and runs on one compute unit
    cm = coarse.reshape(-1, n, Cc)
    cm2 = cm * cm
    out = torch.empty((K, K, K, Ca, Cc), dtype=torch.float64, device=fine.device)
    out2 = torch.empty_like(out)
    span = step * (n - 1) + 1
    for kd in range(K):
        for kh in range(K):
            for kw in range(K):
                v = fp[:, kd:kd + span:step, kh:kh + span:step, kw:kw + span:step, :].reshape(-1, n, Ca).transpose(1, 2)
                out[kd, kh, kw] = torch.bmm(v, cm).sum(0)
                out2[kd, kh, kw] = torch.bmm(v * v, cm2).sum(0)
    return out, out2


def dw_reference(x, dz, ksize, stride=1, transposed=False):
    """x [B, D, D, D, Cin], dz [B, Do, Do, Do, Cout] (Do = D, D / 2 or, transposed, 2 D), any float dtype -> DwRef."""
    x, dz = x.double(), dz.double()
    B, D = x.shape[0], x.shape[1]
    Do = dz.shape[1]
    if transposed:
        assert Do == 2 * D
        pb = max(ksize - 2, 0) // 2
        dk, s2k = _tap_sums(dz, x, ksize, 2, pb, max(ksize - 2, 0) - pb)          # [k, k, k, Cout, Cin]
        n = B * D ** 3
    elif stride == 2:
        assert 2 * Do == D
        pb = max(ksize - 2, 0) // 2
        dk, s2k = _tap_sums(x, dz, ksize, 2, pb, max(ksize - 2, 0) - pb)          # [k, k, k, Cin, Cout]
        n = B * Do ** 3
    else:
        assert stride == 1 and Do == D and ksize % 2 == 1
        pad = (ksize - 1) // 2
        dk, s2k = _tap_sums(x, dz, ksize, 1, pad, pad)
        n = B * D ** 3
    flat = dz.reshape(-1, dz.shape[-1])
    return DwRef(dk, flat.sum(0), s2k, (flat * flat).sum(0), n, B * Do ** 3)
