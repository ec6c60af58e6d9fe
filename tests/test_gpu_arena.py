"""-m gpu: no hot-path kernel touches memory outside its buffers.

Every case below is one call of the C ABI (include/pcgc.h) whose operands lie in arenas (tests/_arena.py): pads of at least
1 MiB and one batch element on both sides, finite poison around the inputs, the canary 0xA5 around and inside the outputs,
scratch of exactly the bytes the sizing function reports.  The call runs once on plain allocations and three times on arenas;
the outputs must be the same bytes every time and nothing but the outputs may change (tests/test_arena_host.py shows that the
harness reports a kernel that strays).  The cases are ONE table, ROWS: name, environment, maker of (call, operands).  A new
kernel, entry point or launch form adds a row, not a test.  The shapes are the smallest that select each launch form (read
from the dispatch code, DESIGN.md "Guard bands"), not the workload's.

Also here: the empty calls of the header's line 28 (EMPTY_ROWS) and the top-k edges against oracle.points.
"""
import ctypes
import math
import zlib

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import _arena                                                             # noqa: E402
import _entropy_cases as ec                                               # noqa: E402
from _arena import Case, In, InOut, Out, Scratch                          # noqa: E402
from oracle import points as opoints                                      # noqa: E402
from pcgcv1_amd import _lib, synthetic                                    # noqa: E402
from pcgcv1_amd.models import model_voxception as model                   # noqa: E402

P = _lib.dptr
F32, I32, I16, U8, F64, I64 = torch.float32, torch.int32, torch.int16, torch.uint8, torch.float64, torch.int64
BOUND = 1e-9


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    torch.cuda.set_device(0)


def S():
    return _lib.stream()


def lib():
    return _lib.hip()


def _rng(*key):
    """A generator seeded by the case's own key (crc32 of the strings: the same inputs in every process)."""
    return np.random.default_rng([k if isinstance(k, int) else zlib.crc32(str(k).encode()) for k in key])


def _f(rng, shape, scale=1.0):
    return torch.from_numpy((rng.standard_normal(shape) * scale).astype(np.float32))


def _ptrs(tensors):
    """A C array of device pointers (const float* const* params); the tensors are the operands, the array lives on the host."""
    arr = (ctypes.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])
    return arr, ctypes.cast(arr, ctypes.c_void_p)


ROWS = []            # (name, env, make): make() -> (call, operands); env = environment the library reads per call
EMPTY_ROWS = []      # the same for calls with B = 0 / n = 0 / rows = 0: every operand is a canary-filled arena


def row(name, make, env=None, empty=False):
    (EMPTY_ROWS if empty else ROWS).append(pytest.param(name, env or {}, make, id=name.replace(" ", "_")))


# ----------------------------------------------------------------------------------------------------------------------
# Layers: pcgc_conv3d_fwd.  One shape per kernel family behind it (conv_valu.hip, conv_mfma.hip, conv_direct.hip).
# ----------------------------------------------------------------------------------------------------------------------
LAYERS = [
    # what, Cin, Cout, k, stride, transposed, D, B, algos.  pcgc_conv3d_fwd (net.hip): algo 0 takes the LDS-tiled VALU kernel where
    # Cin or Cout is 1 (conv_valu.hip run_valu), else the MFMA kernel of the shape (conv_mfma.hip launch_conv_mfma), else the
    # direct kernel; algo 1 the direct kernel (conv_direct.hip); algo 3 the VALU tile kernel of a 4 / 8-channel shape.
    ("block layer", 16, 4, 3, 1, 0, 16, 3, (0, 1, 3)),      # 0: row-packed run_conv<16,4,2,2,3,1,2,2>; 3: run_valu<16,4>
    ("conv_in", 1, 16, 3, 1, 0, 16, 3, (0, 1)),              # 0: run_valu<1,16>
    ("deconv_out", 16, 1, 3, 1, 0, 16, 3, (0, 1)),           # 0: run_valu<16,1>
    # launch_conv_mfma: `small` = B * (D/4) * (D/4) * (D/16) < 320 (D the coarse side): below 20 cubes at 16^3 2 x 2-row tiles
    # (run_small / run_tconv_small), from 20 on 4 x 4-row tiles (run_conv / run_tconv)
    ("stride 1 small", 64, 16, 3, 1, 0, 16, 3, (0, 1)),
    ("stride 1 large", 64, 16, 3, 1, 0, 16, 21, (0,)),
    ("stride 2 small", 32, 64, 3, 2, 0, 32, 3, (0, 1)),
    ("stride 2 large", 32, 64, 3, 2, 0, 32, 21, (0,)),
    ("transposed small", 64, 32, 3, 2, 1, 16, 3, (0, 1)),
    ("transposed large", 64, 32, 3, 2, 1, 16, 21, (0,)),
    ("1x1x1 small", 64, 16, 1, 1, 0, 16, 3, (0, 1)),
    ("1x1x1 large", 64, 16, 1, 1, 0, 16, 21, (0,)),
    ("9x9x9 stride 2", 1, 32, 9, 2, 0, 16, 3, (0, 1)),       # no MFMA plan: the direct kernel either way
]


def _conv_fwd(cin, cout, k, stride, tr, D, B, algo, bias_relu, nB=None):
    def make():
        rng = _rng("conv", cin, cout, k, stride, tr, D, B)
        Do = 2 * D if tr else D // stride
        kshape = (k, k, k, cout, cin) if tr else (k, k, k, cin, cout)
        ops = [In("x", _f(rng, (B, D, D, D, cin)), batch=B), In("kernel", _f(rng, kshape, 1.0 / math.sqrt(k ** 3 * cin)))]
        if bias_relu:
            ops.append(In("bias", _f(rng, (cout,))))
        ops.append(Out("y", (B, Do, Do, Do, cout), F32, batch=B))
        n = B if nB is None else nB

        def call(t):
            return lib().pcgc_conv3d_fwd(P(t["x"]), P(t["kernel"]), P(t.get("bias")), P(t["y"]), n, D, cin, cout, k, stride, tr,
                                         int(bias_relu), algo, S())
        return call, ops
    return make


for what, cin, cout, k, stride, tr, D, B, algos in LAYERS:
    for algo in algos:
        for bias_relu in (True, False):
            row("conv3d_fwd %s %dto%d k%d D%d B%d algo%d %s" % (what, cin, cout, k, D, B, algo, "bias+relu" if bias_relu else "linear"),
                _conv_fwd(cin, cout, k, stride, tr, D, B, algo, bias_relu))
row("conv3d_fwd B=0", _conv_fwd(64, 16, 3, 1, 0, 16, 1, 0, True, nB=0), empty=True)


# ----------------------------------------------------------------------------------------------------------------------
# Blocks: pcgc_vrn_fwd.  The three row-kernel stages, the 16^3 stage on both sides of its launch-size threshold, one generic shape.
# ----------------------------------------------------------------------------------------------------------------------
def _block_params(rng, C):
    q, h = C // 4, C // 2
    out = []
    for name, (k, ci, co) in (("conv1_1", (3, C, q)), ("conv1_2", (3, q, h)), ("conv2_1", (1, C, q)), ("conv2_2", (3, q, q)),
                              ("conv2_3", (1, q, h))):
        out += [(name + "_kernel", _f(rng, (k, k, k, ci, co), math.sqrt(2.0 / (k ** 3 * ci)))), (name + "_bias", _f(rng, (co,), 0.1))]
    return out


def _vrn_fwd(C, D, B, alias, nB=None):
    def make():
        rng = _rng("vrn", C, D, B)
        params = _block_params(rng, C)
        x = torch.relu(_f(rng, (B, D, D, D, C)))
        n = B if nB is None else nB
        nbytes = int(lib().pcgc_vrn_workspace_bytes(n, D, C))
        ops = [In(k, v) for k, v in params] + [Scratch("workspace", nbytes)]
        ops += [InOut("x_out", x, batch=B)] if alias else [In("x", x, batch=B), Out("out", x.shape, F32, batch=B)]

        def call(t):
            keep, arr = _ptrs([t[k] for k, _ in params])
            xin, out = (t["x_out"], t["x_out"]) if alias else (t["x"], t["out"])
            return lib().pcgc_vrn_fwd(P(xin), arr, P(out), n, D, C, P(t["workspace"]), nbytes, S())
        return call, ops
    return make


for C, D, B in ((16, 64, 1), (32, 32, 3), (64, 16, 5), (64, 16, 21), (64, 16, 33), (8, 16, 2)):
    for alias in (False, True):
        row("vrn_fwd C%d D%d B%d %s" % (C, D, B, "in place" if alias else "out apart"), _vrn_fwd(C, D, B, alias))
# The 32^3 and 16^3 row kernels pick their wave tile by launch size, and switches read per launch force one
# (test_tiles_chosen_by_launch_size_do_not_change_a_bit).
#   vrn_row32.hip launch_vrn32_row: up to 16 cubes vrn32a_row_kernel<1,2> / vrn32bc_row_kernel<2> and NO switch is read; from 17
#     cubes kernel A runs <1,4> (below 56 cubes), <2,8> (PCGC_A32_TILE=28: 56 cubes and more) or <2,4> (=24); kernel BC of a
#     pcgc_vrn_fwd call (x of any sign) is <8>.  The dense BC forms <4>, <16>, <8> on a non-negative x and the skipping forms
#     are the nets' (synthesis and analysis rows at 17 cubes below).
#   vrn_row16.hip launch_vrn64_row: 1 plane per wave up to 32 cubes, 2 from 33, 4 from 128; PCGC_V64_LD forces one at any size.
TILES = ({"PCGC_A32_TILE": "28", "PCGC_BC32_LD": "16", "PCGC_DOWN2_LD": "4", "PCGC_V64_LD": "4"},
         {"PCGC_A32_TILE": "24", "PCGC_BC32_LD": "8", "PCGC_DOWN2_LD": "2", "PCGC_V64_LD": "2"})
for alias in (False, True):
    row("vrn_fwd C32 D32 B17 %s" % ("in place" if alias else "out apart"), _vrn_fwd(32, 32, 17, alias))
for i, env in enumerate(TILES):
    row("vrn_fwd C32 D32 B17 in place, A32 tile %s" % env["PCGC_A32_TILE"], _vrn_fwd(32, 32, 17, True), env=env)
    row("vrn_fwd C64 D16 B3 in place, %s planes per wave" % env["PCGC_V64_LD"], _vrn_fwd(64, 16, 3, True), env=env)
row("vrn_fwd B=0", _vrn_fwd(64, 16, 1, False, nB=0), empty=True)


# ----------------------------------------------------------------------------------------------------------------------
# Whole nets: pcgc_net_forward, workspace exactly pcgc_net_workspace_bytes.
# ----------------------------------------------------------------------------------------------------------------------
_NETS = {}


def _net(kind):
    """One net per kind for the module (synthetic dense weights): the weights are the library's own copy, not an operand."""
    if not _NETS:
        w = synthetic.make_weights(seed=41, profile="dense")
        for cls in (model.AnalysisTransform, model.SynthesisTransform, model.HyperEncoder, model.HyperDecoder):
            _NETS[cls.net_name] = cls().load_weights(w)
    return _NETS[kind]


def _net_forward(kind, B, nB=None):
    def make():
        net = _net(kind)
        rng = _rng("net", kind, B)
        if kind == "analysis_transform":
            D, x = 64, torch.from_numpy(synthetic.make_cubes(seed=43, n_cubes=B))
        elif kind == "hyper_decoder":
            D, x = 8, torch.round(_f(rng, (B, 8, 8, 8, 8), 2.0))
        else:
            D, x = 16, torch.round(_f(rng, (B, 16, 16, 16, 16), 2.0))
        cin, cout, dout = net._geometry(D)
        n = B if nB is None else nB
        _lib.check(lib().pcgc_net_set_algo(net._handle, 0))
        nbytes = int(lib().pcgc_net_workspace_bytes(net._handle, n, D))
        n_out = 2 if kind == "hyper_decoder" else 1
        ops = [In("x", x, batch=B), Scratch("workspace", nbytes)] + [Out("out%d" % i, (B, dout, dout, dout, cout), F32, batch=B) for i in range(n_out)]

        def call(t):
            return lib().pcgc_net_forward(net._handle, P(t["x"]), P(t["out0"]), P(t.get("out1")), n, D, BOUND, P(t["workspace"]),
                                          nbytes, S())
        return call, ops
    return make


# net.hip, pcgc_net_forward: PCGC_SKIP_EMPTY 3 (default) = the 64^3 blocks on slots (vrn_seg.hip), 1 = whole-row tiles that are
# not written, 0 = every tile computed.  On slots the kernels read the empty-cube responses through one 2 GiB window: in place
# where the net's blob lies within reach of the chunk, else (or with PCGC_SEG_COPY_EMPTY=1) from a copy behind the scratch.
row("net_forward analysis B3 slots", _net_forward("analysis_transform", 3))
row("net_forward analysis B3 slots, responses copied", _net_forward("analysis_transform", 3), env={"PCGC_SEG_COPY_EMPTY": "1"})
row("net_forward analysis B3 row tiles", _net_forward("analysis_transform", 3), env={"PCGC_SKIP_EMPTY": "1"})
row("net_forward analysis B3 no skipping", _net_forward("analysis_transform", 3), env={"PCGC_SKIP_EMPTY": "0"})
row("net_forward synthesis B3", _net_forward("synthesis_transform", 3))
# 17 cubes: one more than the small-launch forms of the 32^3 stage take (the stage's chunk is 64 cubes, net_plan.h chunk_plan).
# Synthesis (dense, x non-negative): A <1,4> and BC <4> by default, <2,8> and <16>, <2,4> and <8> forced.  Analysis: the
# skipping forms vrn32a_row_kernel<2,4,false,false> and vrn32bc_row_kernel<8,false,true>; of the switches it reads
# PCGC_DOWN2_LD and PCGC_V64_LD.
for kind, what in (("analysis_transform", "analysis B17 slots"), ("synthesis_transform", "synthesis B17")):
    row("net_forward %s" % what, _net_forward(kind, 17))
    for env in TILES:
        row("net_forward %s, tiles %s" % (what, "/".join(env[k] for k in sorted(env))), _net_forward(kind, 17), env=env)
for B in (1, 65):       # hyper_row.hip planes_per_wave: 1 plane per wave, and 2 (four-wave kernels) / 1 (<16,8>) past 64 cubes
    row("net_forward hyper encoder B%d" % B, _net_forward("hyper_encoder", B))
    row("net_forward hyper decoder B%d" % B, _net_forward("hyper_decoder", B))
for kind in ("analysis_transform", "synthesis_transform", "hyper_encoder", "hyper_decoder"):
    row("net_forward %s B=0" % kind, _net_forward(kind, 1, nB=0), empty=True)


def _rowocc(B, nB=None):
    def make():
        x = torch.from_numpy(synthetic.make_cubes(seed=47, n_cubes=B))
        n = B if nB is None else nB

        def call(t):
            return lib().pcgc_rowocc(P(t["x"]), P(t["rowocc"]), n, S())
        return call, [In("x", x, batch=B), Out("rowocc", (B * 64,), I64, batch=B)]
    return make


row("rowocc B3", _rowocc(3))
row("rowocc B=0", _rowocc(1, nB=0), empty=True)


# ----------------------------------------------------------------------------------------------------------------------
# Entropy kernels and the coder boundary (entropy.hip).  Lengths that are no multiple of a workgroup.
# ----------------------------------------------------------------------------------------------------------------------
LENGTHS = ((3 * 4096 + 1, 3 * 4096 + 1), (5 * 777, 777))          # (n, seg_len)


def _round_minmax(n, seg_len, i16, nn=None):
    def make():
        x = _f(_rng("round", n), (n,), 3.0)
        cnt = n if nn is None else nn
        fn = lib().pcgc_round_minmax_i16 if i16 else lib().pcgc_round_minmax
        ops = [In("x", x), Out("q", (n,), I16 if i16 else F32), Out("seg_min", (n // seg_len,), I32), Out("seg_max", (n // seg_len,), I32)]
        return (lambda t: fn(P(t["x"]), P(t["q"]), P(t["seg_min"]), P(t["seg_max"]), cnt, seg_len, S())), ops
    return make


def _symbols(n, seg_len, seg, nn=None):
    def make():
        rng = _rng("sym", n)
        sym = torch.from_numpy(rng.integers(-300, 300, n).astype(np.int16))
        cnt = n if nn is None else nn
        if seg:
            offs = torch.from_numpy(rng.integers(-9, 9, n // seg_len).astype(np.float32))
            return (lambda t: lib().pcgc_symbols_to_values_seg(P(t["sym"]), P(t["seg_offset"]), P(t["out"]), cnt, seg_len, S())), \
                [In("sym", sym), In("seg_offset", offs), Out("out", (n,), F32)]
        return (lambda t: lib().pcgc_symbols_to_values(P(t["sym"]), -7, P(t["out"]), cnt, S())), [In("sym", sym), Out("out", (n,), F32)]
    return make


def _laplace_likelihood(n, noise, nn=None):
    def make():
        rng = _rng("laplace", n)
        ops = [In("y", _f(rng, (n,), 2.0)), In("loc", _f(rng, (n,), 0.7)), In("scale", _f(rng, (n,), 0.8).abs().clamp_min(1e-9))]
        if noise:
            ops.append(In("noise", torch.from_numpy((rng.random(n) - 0.5).astype(np.float32))))
        ops += [Out("values", (n,), F32), Out("likelihood", (n,), F32)]
        cnt = n if nn is None else nn
        return (lambda t: lib().pcgc_laplace_likelihood(P(t["y"]), P(t["loc"]), P(t["scale"]), P(t.get("noise")), P(t["values"]),
                                                        P(t["likelihood"]), cnt, BOUND, S())), ops
    return make


def _factorized_likelihood(n, C, noise, nn=None):
    def make():
        rng = _rng("factorized", n, C)
        ops = [In("z", _f(rng, (n // C, C), 2.0)), In("params", torch.tensor(ec.factorized_params(C)[1]))]
        if noise:
            ops.append(In("noise", torch.from_numpy((rng.random((n // C, C)) - 0.5).astype(np.float32))))
        ops += [Out("values", (n // C, C), F32), Out("likelihood", (n // C, C), F32)]
        cnt = n if nn is None else nn
        return (lambda t: lib().pcgc_factorized_likelihood(P(t["z"]), P(t["params"]), P(t.get("noise")), P(t["values"]), P(t["likelihood"]),
                                                           cnt, C, BOUND, S())), ops
    return make


def _factorized_pmf(C, lo, hi):
    def make():
        return (lambda t: lib().pcgc_factorized_pmf(P(t["params"]), C, lo, hi, BOUND, P(t["pmf"]), S())), \
            [In("params", torch.tensor(ec.factorized_params(C)[1])), Out("pmf", (C, hi - lo + 1), F32)]
    return make


def _laplace_cdf(ncols, want_cdf, want_lohi, rows=5 * 777, seg_rows=777, nrows=None):
    def make():
        rng = _rng("cdf", ncols)
        nseg = rows // seg_rows
        width = rng.integers(1, ncols + 1, nseg)                 # segments narrower than ncols too
        width[0], width[-1] = ncols, 1
        mn = np.array([-(w // 2) for w in width], np.int32)
        mx = (mn + width - 1).astype(np.int32)
        rmin, rmax = np.repeat(mn, seg_rows), np.repeat(mx, seg_rows)
        ops = [In("loc", _f(rng, (rows,), 2.0)), In("scale", torch.from_numpy(np.exp(rng.uniform(np.log(0.05), np.log(30.0), rows)).astype(np.float32))),
               In("seg_min", torch.from_numpy(mn)), In("seg_max", torch.from_numpy(mx))]
        if want_lohi:
            ops += [In("symbols", torch.from_numpy(rng.integers(rmin, rmax + 1).astype(np.float32))), Out("lohi", (rows,), I32)]
        if want_cdf:
            ops.append(Out("cdf_lower", (rows, ncols), I16))
        cnt = rows if nrows is None else nrows
        return (lambda t: lib().pcgc_laplace_cdf(P(t["loc"]), P(t["scale"]), P(t["seg_min"]), P(t["seg_max"]), cnt, seg_rows, ncols, BOUND,
                                                 P(t.get("symbols")), P(t.get("cdf_lower")), P(t.get("lohi")), S())), ops
    return make


for n, seg_len in LENGTHS:
    row("round_minmax n%d seg%d" % (n, seg_len), _round_minmax(n, seg_len, False))
    row("round_minmax_i16 n%d seg%d" % (n, seg_len), _round_minmax(n, seg_len, True))
    row("symbols_to_values n%d" % n, _symbols(n, seg_len, False))
    row("symbols_to_values_seg n%d seg%d" % (n, seg_len), _symbols(n, seg_len, True))
    for noise in (False, True):
        row("laplace_likelihood n%d %s" % (n, "noise" if noise else "rounded"), _laplace_likelihood(n, noise))
        # whole rows of C = 8 channels: the next multiple of 8 (1537 and 486 rows: no multiple of a workgroup either)
        row("factorized_likelihood n%d C8 %s" % (-(-n // 8) * 8, "noise" if noise else "rounded"), _factorized_likelihood(-(-n // 8) * 8, 8, noise))
row("factorized_pmf C8 -15..15", _factorized_pmf(8, -15, 15))
row("factorized_pmf C3 -2..1", _factorized_pmf(3, -2, 1))
for ncols in (4, 8, 14, 31):                                # laplace_cdf_kernel<4>, <8>, <16>, <32> (tests/test_gpu_entropy_forms.py)
    row("laplace_cdf ncols%d cdf" % ncols, _laplace_cdf(ncols, True, False))
    row("laplace_cdf ncols%d lohi" % ncols, _laplace_cdf(ncols, False, True))
row("laplace_cdf ncols8 one-row segments, both outputs", _laplace_cdf(8, True, True, rows=1000, seg_rows=1))
row("round_minmax n=0", _round_minmax(777, 777, False, nn=0), empty=True)
row("round_minmax_i16 n=0", _round_minmax(777, 777, True, nn=0), empty=True)
row("symbols_to_values n=0", _symbols(777, 777, False, nn=0), empty=True)
row("symbols_to_values_seg n=0", _symbols(777, 777, True, nn=0), empty=True)
row("laplace_likelihood n=0", _laplace_likelihood(777, True, nn=0), empty=True)
row("factorized_likelihood n=0", _factorized_likelihood(776, 8, True, nn=0), empty=True)
row("laplace_cdf rows=0", _laplace_cdf(8, True, True, nrows=0), empty=True)


# ----------------------------------------------------------------------------------------------------------------------
# Tail (tail.hip): top-k, voxelisation, loss sums.
# ----------------------------------------------------------------------------------------------------------------------
TAIL = ((3, 64), (2, 8))


def _topk(B, cs, want_mask, fixed, nB=None):
    def make():
        vox = cs ** 3
        rng = _rng("topk", B, cs)
        x = _f(rng, (B, vox), 3.0)
        k = torch.from_numpy(rng.integers(1, vox // 20 + 2, B).astype(np.int32))
        n = B if nB is None else nB
        nbytes = int(lib().pcgc_topk_workspace_bytes(n, vox))
        ops = [In("x", x, batch=B), In("k_per_cube", k), Out("thresholds", (B,), F32), Scratch("workspace", nbytes)]
        if want_mask:
            ops.append(Out("mask", (B, vox), U8, batch=B))
        return (lambda t: lib().pcgc_topk_threshold(P(t["x"]), P(t["k_per_cube"]), n, vox, int(fixed), 0.25, P(t["thresholds"]),
                                                    P(t.get("mask")), P(t["workspace"]), nbytes, S())), ops
    return make


def _voxelize_points(B, cs):
    def make():
        rng = _rng("voxelize", B, cs)
        n = 4099
        pts = torch.from_numpy(rng.integers(0, 4 * cs, (n, 3)).astype(np.int32))
        cop = torch.from_numpy(rng.integers(-1, B + 2, n).astype(np.int32))          # -1: a dropped cube; B, B + 1: another rank's
        return (lambda t: lib().pcgc_voxelize_points(P(t["points"]), P(t["cube_of_point"]), n, cs, 0, B, P(t["cubes"]), S())), \
            [In("points", pts), In("cube_of_point", cop), InOut("cubes", torch.zeros((B, cs, cs, cs, 1)), batch=B)]
    return make


def _bce_sums(B, cs):
    def make():
        n = B * cs ** 3
        rng = _rng("bce", n)
        nbytes = int(lib().pcgc_bce_workspace_bytes(n))
        return (lambda t: lib().pcgc_bce_sums(P(t["pred"]), P(t["label"]), n, P(t["sums4"]), P(t["workspace"]), nbytes, S())), \
            [In("pred", _f(rng, (n,), 2.0)), In("label", torch.from_numpy((rng.random(n) < 0.02).astype(np.float32))), Out("sums4", (4,), F64),
             Scratch("workspace", nbytes)]
    return make


def _train_loss_sums(B, cs):
    def make():
        n, ny, nz = B * cs ** 3, B * (cs // 4) ** 3 * 16 + 1, B * (cs // 8) ** 3 * 8 + 3
        rng = _rng("loss sums", n)
        nbytes = int(lib().pcgc_train_loss_sums_workspace_bytes(n))
        lik = lambda m: torch.from_numpy(rng.uniform(1e-9, 1.0, m).astype(np.float32))                      # noqa: E731
        return (lambda t: lib().pcgc_train_loss_sums(P(t["pred"]), P(t["label"]), n, P(t["lik_y"]), ny, P(t["lik_z"]), nz, P(t["sums4"]),
                                                     P(t["logs2"]), P(t["workspace"]), nbytes, S())), \
            [In("pred", _f(rng, (n,), 2.0)), In("label", torch.from_numpy((rng.random(n) < 0.02).astype(np.float32))), In("lik_y", lik(ny)),
             In("lik_z", lik(nz)), Out("sums4", (4,), F64), Out("logs2", (2,), F64), Scratch("workspace", nbytes)]
    return make


for B, cs in TAIL:
    row("topk_threshold B%d %d^3 thresholds and mask" % (B, cs), _topk(B, cs, True, False))
    row("topk_threshold B%d %d^3 thresholds alone" % (B, cs), _topk(B, cs, False, False))
    row("topk_threshold B%d %d^3 fixed threshold" % (B, cs), _topk(B, cs, True, True))
    row("voxelize_points B%d %d^3" % (B, cs), _voxelize_points(B, cs))
    row("bce_sums B%d %d^3" % (B, cs), _bce_sums(B, cs))
    row("train_loss_sums B%d %d^3" % (B, cs), _train_loss_sums(B, cs))
row("topk_threshold B=0", _topk(1, 8, True, False, nB=0), empty=True)


# ----------------------------------------------------------------------------------------------------------------------
# Training, layer level (train.hip bwd_data_impl / bwd_weight_impl).  Workspace exactly pcgc_conv3d_bwd_workspace_bytes.
# ----------------------------------------------------------------------------------------------------------------------
BWD_DATA = [
    # which branch of bwd_data_impl the adjoint convolution takes; Cin, Cout, k, stride, transposed, D, B of the LAYER
    ("VALU", 16, 4, 3, 1, 0, 16, 3),                          # adjoint 4 -> 16: launch_conv_valu run_valu<4,16>
    ("MFMA mode 0", 64, 16, 3, 1, 0, 16, 3),                  # adjoint 16 -> 64 on the flipped filter
    ("MFMA mode 1", 64, 32, 3, 2, 1, 16, 3),                  # a transposed layer's adjoint is the stride-2 conv
    ("MFMA mode 2", 32, 64, 3, 2, 0, 32, 3),                  # a stride-2 layer's adjoint is the transposed conv
    ("hyper 8^3 16to8", 16, 8, 3, 1, 0, 8, 3),                # adjoint 8 -> 16 at 8^3: conv8_row_kernel<8,16> + mask_add_kernel
    ("hyper 8^3 8to16", 8, 16, 3, 1, 0, 8, 3),                # adjoint 16 -> 8: conv8_row_kernel<16,8>
    ("hyper down", 16, 16, 3, 2, 1, 8, 3),                    # transposed 8 -> 16: adjoint = down8_row_kernel
    ("hyper up", 16, 16, 3, 2, 0, 16, 3),                     # stride 2 16 -> 8: adjoint = up8_row_kernel
    ("direct", 1, 32, 9, 2, 0, 16, 3),
]


def _bwd_data(cin, cout, k, stride, tr, D, B, form):
    """form: plain (pcgc_conv3d_bwd_data), mask, add_to, add_to aliasing dx (pcgc_conv3d_bwd_data_fused)."""
    def make():
        rng = _rng("bwd_data", cin, cout, k, stride, tr, D)
        Do = 2 * D if tr else D // stride
        kshape = (k, k, k, cout, cin) if tr else (k, k, k, cin, cout)
        nbytes = int(lib().pcgc_conv3d_bwd_workspace_bytes(cin, cout, k))
        xs = (B, D, D, D, cin)
        ops = [In("dz", _f(rng, (B, Do, Do, Do, cout)), batch=B), In("kernel", _f(rng, kshape, 0.2)), Scratch("workspace", nbytes)]
        if form == "mask":
            ops.append(In("relu_mask", _f(rng, xs), batch=B))
        if form == "add_to":
            ops.append(In("add_to", _f(rng, xs), batch=B))
        ops.append(InOut("dx", _f(rng, xs), batch=B) if form == "add_to aliasing dx" else Out("dx", xs, F32, batch=B))

        def call(t):
            if form == "plain":
                return lib().pcgc_conv3d_bwd_data(P(t["dz"]), P(t["kernel"]), P(t["dx"]), B, D, cin, cout, k, stride, tr, P(t["workspace"]),
                                                  nbytes, S())
            add = t["dx"] if form == "add_to aliasing dx" else t.get("add_to")
            return lib().pcgc_conv3d_bwd_data_fused(P(t["dz"]), P(t["kernel"]), P(t["dx"]), P(t.get("relu_mask")), P(add), B, D, cin, cout, k,
                                                    stride, tr, P(t["workspace"]), nbytes, S())
        return call, ops
    return make


for what, cin, cout, k, stride, tr, D, B in BWD_DATA:
    for form in ("plain", "mask", "add_to", "add_to aliasing dx"):
        row("conv3d_bwd_data %s %dto%d k%d D%d %s" % (what, cin, cout, k, D, form), _bwd_data(cin, cout, k, stride, tr, D, B, form))

# pcgc_net_forward hands the hyper nets' 8^3 kernels at most kHyperChunk = 256 cubes (net_plan.h), so conv8_row_kernel<16,8>
# (two waves per cube) never runs at 8 planes per wave there.  This entry point passes B whole: from 512 cubes 8 planes per
# wave, and 513 cubes are the one launch whose last workgroup is half empty (1026 waves, four to a workgroup).
for B in (512, 513):
    row("conv3d_bwd_data hyper 8^3 8to16 k3 D8 B%d plain" % B, _bwd_data(8, 16, 3, 1, 0, 8, B, "plain"))
    row("conv3d_bwd_data hyper 8^3 8to16 k3 D8 B%d mask" % B, _bwd_data(8, 16, 3, 1, 0, 8, B, "mask"))

BWD_WEIGHT = [
    # which branch of bwd_weight_impl; k, Cin, Cout, stride, transposed, D, B
    ("tiled", 3, 64, 16, 1, 0, 16, 3),                        # launch_conv_dw_tile: dw_plan.h kMfma_16x16, four channel chunks
    ("tiled 1x1x1", 1, 64, 16, 1, 0, 16, 3),                  # kTile1_16x16
    ("tiled edge", 3, 1, 16, 1, 0, 16, 3),                     # kEdge_1x16
    ("stride 2", 3, 16, 32, 2, 0, 32, 3),                     # launch_conv_dw_tile_s2, x on the fine grid
    ("transposed", 3, 64, 32, 2, 1, 16, 3),                   # launch_conv_dw_tile_s2, dz on the fine grid
    ("generic", 3, 8, 32, 1, 0, 16, 3),                       # conv_dw_partial_kernel<1> (256 weight pairs): no row in dw_plan.h
    ("generic 5x5x5 stride 2", 5, 32, 32, 2, 0, 8, 3),        # conv_dw_partial_kernel<4> (1024 pairs), mode 1
    ("generic 9x9x9", 9, 1, 32, 2, 0, 16, 3),                 # conv_dw_partial_kernel<1>
]


def _bwd_weight(k, cin, cout, stride, tr, D, B, dbias):
    def make():
        rng = _rng("bwd_weight", cin, cout, k, stride, tr, D)
        Do = 2 * D if tr else D // stride
        kshape = (k, k, k, cout, cin) if tr else (k, k, k, cin, cout)
        nbytes = int(lib().pcgc_conv3d_bwd_workspace_bytes(cin, cout, k))
        ops = [In("x", _f(rng, (B, D, D, D, cin)), batch=B), In("dz", _f(rng, (B, Do, Do, Do, cout)), batch=B), Out("dkernel", kshape, F32),
               Scratch("workspace", nbytes)]
        if dbias:
            ops.append(Out("dbias", (cout,), F32))
        return (lambda t: lib().pcgc_conv3d_bwd_weight(P(t["x"]), P(t["dz"]), P(t["dkernel"]), P(t.get("dbias")), B, D, cin, cout, k, stride, tr,
                                                       P(t["workspace"]), nbytes, S())), ops
    return make


for what, k, cin, cout, stride, tr, D, B in BWD_WEIGHT:
    for dbias in (True, False):
        row("conv3d_bwd_weight %s k%d %dto%d D%d %s" % (what, k, cin, cout, D, "with dbias" if dbias else "no dbias"),
            _bwd_weight(k, cin, cout, stride, tr, D, B, dbias))


# ----------------------------------------------------------------------------------------------------------------------
# Training, fused blocks (vrn_row.hip / vrn_row32.hip on the training tensors), where *_supported says so.
# ----------------------------------------------------------------------------------------------------------------------
FUSED = ((64, 16, 1), (32, 32, 2))                           # D, C, B


def _vrn_fwd_train(D, C, B, form):
    """form: full (pre kept), signs, q4 (signs on Q4 tensors: a permutation of the same voxels, any values do)."""
    def make():
        supported = {"full": lib().pcgc_vrn_fwd_train_supported, "signs": lib().pcgc_vrn_fwd_train_signs_supported,
                     "q4": lib().pcgc_vrn_fwd_train_signs_supported}[form]
        assert supported(D, C) == 1, "no fused forward kernel for D=%d C=%d" % (D, C)
        rng = _rng("fwd_train", D, C)
        params = [(n, v * (0.5 if "kernel" in n else 1.0)) for n, v in _block_params(rng, C)]
        xs, qs = (B, D, D, D, C), (B, D, D, D, C // 4)
        ops = [In(n, v) for n, v in params] + [In("x", torch.relu(_f(rng, xs)), batch=B)]
        ops += [Out(n, qs, F32, batch=B) for n in ("t11", "t21", "t22")]
        ops.append(Out("pre", xs, F32, batch=B) if form == "full" else Out("pre_signs", (B, D, D, D), I32, batch=B))
        ops.append(Out("out", xs, F32, batch=B))
        fn = {"full": lib().pcgc_vrn_fwd_train, "signs": lib().pcgc_vrn_fwd_train_signs, "q4": lib().pcgc_vrn_fwd_train_q4}[form]

        def call(t):
            keep, arr = _ptrs([t[n] for n, _ in params])
            return fn(P(t["x"]), arr, P(t["t11"]), P(t["t21"]), P(t["t22"]), P(t["pre" if form == "full" else "pre_signs"]), P(t["out"]),
                      B, D, C, S())
        return call, ops
    return make


def _vrn_bwd_input(D, C, B, q4, mask):
    def make():
        assert lib().pcgc_vrn_bwd_input_supported(D, C) == 1, "no fused bwd-input kernel for D=%d C=%d" % (D, C)
        rng = _rng("bwd_input", D, C)
        xs, qs = (B, D, D, D, C), (B, D, D, D, C // 4)
        ops = [In("dt11", _f(rng, qs), batch=B), In("dt21", _f(rng, qs), batch=B), InOut("dpre_dx", _f(rng, xs), batch=B),
               In("kernel11", _f(rng, (3, 3, 3, C, C // 4), 0.1)), In("kernel21", _f(rng, (1, 1, 1, C, C // 4), 0.3))]
        if mask:
            ops.append(In("x_mask", _f(rng, xs), batch=B))
        fn = lib().pcgc_vrn_bwd_input_q4 if q4 else lib().pcgc_vrn_bwd_input
        # in place on dpre, as the step calls it
        return (lambda t: fn(P(t["dt11"]), P(t["dt21"]), P(t["dpre_dx"]), P(t.get("x_mask")), P(t["kernel11"]), P(t["kernel21"]), P(t["dpre_dx"]),
                             B, D, C, S())), ops
    return make


def _tail_weights(rng, C):
    Q, H = C // 4, C // 2
    return [In("kernel12", _f(rng, (3, 3, 3, Q, H), 0.1)), In("kernel22", _f(rng, (3, 3, 3, Q, Q), 0.15)), In("kernel23", _f(rng, (1, 1, 1, Q, H), 0.3))]


def _vrn_bwd_tail(D, C, B):
    def make():
        assert lib().pcgc_vrn_bwd_tail_supported(D, C) == 1, "no fused bwd-tail kernel for D=%d C=%d" % (D, C)
        rng = _rng("bwd_tail", D, C)
        hs, qs = (B, D, D, D, C // 2), (B, D, D, D, C // 4)
        ins = [In(n, _f(rng, hs), batch=B) for n in ("dz12", "dz23")] + [In(n, _f(rng, qs), batch=B) for n in ("t11", "t21", "t22")] + _tail_weights(rng, C)
        outs = [Out(n, qs, F32, batch=B) for n in ("dt11", "dt21", "dt22")]
        return (lambda t: lib().pcgc_vrn_bwd_tail(*[P(t[o.name]) for o in ins + outs], B, D, C, S())), ins + outs
    return make


def _vrn_bwd_tail_split(D, C, B, q4):
    def make():
        assert lib().pcgc_vrn_bwd_tail_split_supported(D, C) == 1, "no one-pass bwd-tail kernel for D=%d C=%d" % (D, C)
        rng = _rng("bwd_tail_split", D, C)
        hs, qs = (B, D, D, D, C // 2), (B, D, D, D, C // 4)
        t = {n: _f(rng, qs) for n in ("t11", "t21", "t22")}
        signs = torch.from_numpy(rng.integers(0, 1 << 16, (B, D, D, D)).astype(np.int32))
        for base, n in ((16, "t22"), (20, "t11"), (24, "t21")):            # the masks the forward kernel leaves in bits 16-27
            for i in range(4):
                signs |= (t[n][..., i] > 0).to(I32) << (base + i)
        ins = [In("dout", _f(rng, (B, D, D, D, C)), batch=B), In("pre_signs", signs, batch=B)] + [In(n, t[n], batch=B) for n in ("t11", "t21", "t22")]
        ins += _tail_weights(rng, C)
        outs = [Out(n, hs, F32, batch=B) for n in ("dz12", "dz23")] + [Out(n, qs, F32, batch=B) for n in ("dt11", "dt21", "dt22")]
        fn = lib().pcgc_vrn_bwd_tail_split_q4 if q4 else lib().pcgc_vrn_bwd_tail_split
        return (lambda b: fn(*[P(b[o.name]) for o in ins + outs], B, D, C, S())), ins + outs
    return make


for D, C, B in FUSED:
    row("vrn_fwd_train D%d C%d B%d" % (D, C, B), _vrn_fwd_train(D, C, B, "full"))
    row("vrn_fwd_train_signs D%d C%d B%d" % (D, C, B), _vrn_fwd_train(D, C, B, "signs"))
    for mask in (True, False):
        row("vrn_bwd_input D%d C%d B%d in place%s" % (D, C, B, ", x_mask" if mask else ""), _vrn_bwd_input(D, C, B, False, mask))
    row("vrn_bwd_tail D%d C%d B%d" % (D, C, B), _vrn_bwd_tail(D, C, B))
# the Q4 layout and the one-pass tail exist for the 64^3 stage only (pcgc.h)
row("vrn_fwd_train_q4 D64 C16 B1", _vrn_fwd_train(64, 16, 1, "q4"))
for mask in (True, False):
    row("vrn_bwd_input_q4 D64 C16 B1 in place%s" % (", x_mask" if mask else ""), _vrn_bwd_input(64, 16, 1, True, mask))
row("vrn_bwd_tail_split D64 C16 B1", _vrn_bwd_tail_split(64, 16, 1, False))
row("vrn_bwd_tail_split_q4 D64 C16 B1", _vrn_bwd_tail_split(64, 16, 1, True))


# ----------------------------------------------------------------------------------------------------------------------
# Training, elementwise kernels and reductions.
# ----------------------------------------------------------------------------------------------------------------------
def _elementwise(name, n):
    """name -> maker; n = voxels (the per-voxel kernels) or elements."""
    def make():
        rng = _rng(name, n)
        C, H = 16, 8
        L = lib()
        if name == "relu_bwd":                                 # a channel slice of dy: stride 16, offset 8
            return (lambda t: L.pcgc_relu_bwd(P(t["dy"]), 16, 8, P(t["y"]), P(t["dz"]), n, H, S())), \
                [In("dy", _f(rng, (n, 16))), In("y", _f(rng, (n, H))), Out("dz", (n, H), F32)]
        if name == "relu_bwd copy":
            return (lambda t: L.pcgc_relu_bwd(P(t["dy"]), 16, 8, None, P(t["dz"]), n, H, S())), [In("dy", _f(rng, (n, 16))), Out("dz", (n, H), F32)]
        if name == "vrn_merge":
            return (lambda t: L.pcgc_vrn_merge(P(t["x"]), P(t["t12"]), P(t["t23"]), P(t["out"]), n, C, S())), \
                [In("x", _f(rng, (n, C))), In("t12", _f(rng, (n, H))), In("t23", _f(rng, (n, H))), Out("out", (n, C), F32)]
        if name in ("vrn_bwd_split", "vrn_bwd_split premasked"):
            pm = int(name.endswith("premasked"))
            ops = [In("dout", _f(rng, (n, C))), In("out", _f(rng, (n, C))), In("t12", _f(rng, (n, H))), In("t23", _f(rng, (n, H)))]
            ops += ([] if pm else [Out("dpre", (n, C), F32)]) + [Out("dz12", (n, H), F32), Out("dz23", (n, H), F32)]
            return (lambda t: L.pcgc_vrn_bwd_split(P(t["dout"]), P(t["out"]), P(t["t12"]), P(t["t23"]), P(t.get("dpre")), P(t["dz12"]), P(t["dz23"]),
                                                   n, C, pm, S())), ops
        if name == "vrn_bwd_split_signs":
            signs = torch.from_numpy(rng.integers(0, 1 << 16, n).astype(np.int32))
            return (lambda t: L.pcgc_vrn_bwd_split_signs(P(t["dout"]), P(t["out"]), P(t["pre_signs"]), P(t["dpre"]), P(t["dz12"]), P(t["dz23"]),
                                                         n, C, 0, S())), \
                [In("dout", _f(rng, (n, C))), In("out", _f(rng, (n, C))), In("pre_signs", signs), Out("dpre", (n, C), F32),
                 Out("dz12", (n, H), F32), Out("dz23", (n, H), F32)]
        if name == "abs_max":
            return (lambda t: L.pcgc_abs_max(P(t["s_raw"]), 0.11, None, P(t["out"]), n, S())), [In("s_raw", _f(rng, (n,))), Out("out", (n,), F32)]
        if name == "abs_max gradient":
            return (lambda t: L.pcgc_abs_max(P(t["s_raw"]), 0.11, P(t["dscale"]), P(t["out"]), n, S())), \
                [In("s_raw", _f(rng, (n,))), In("dscale", _f(rng, (n,))), Out("out", (n,), F32)]
        if name == "add_inplace":
            return (lambda t: L.pcgc_add_inplace(P(t["a"]), P(t["b"]), n, S())), [InOut("a", _f(rng, (n,))), In("b", _f(rng, (n,)))]
        if name == "laplace_likelihood_bwd":
            return (lambda t: L.pcgc_laplace_likelihood_bwd(P(t["values"]), P(t["loc"]), P(t["scale"]), -0.37, BOUND, P(t["dvalues"]), P(t["dloc"]),
                                                            P(t["dscale"]), n, S())), \
                [In("values", _f(rng, (n,), 2.0)), In("loc", _f(rng, (n,), 0.7)), In("scale", _f(rng, (n,), 0.8).abs().clamp_min(1e-3)),
                 Out("dvalues", (n,), F32), Out("dloc", (n,), F32), Out("dscale", (n,), F32)]
        if name.startswith("factorized_likelihood_bwd"):
            Cf = int(name.split("C")[1])                        # n values = n / Cf rows of Cf channels
            m = n * Cf
            nbytes = int(L.pcgc_factorized_bwd_workspace_bytes(Cf))
            return (lambda t: L.pcgc_factorized_likelihood_bwd(P(t["values"]), P(t["params"]), -0.37, BOUND, P(t["dvalues"]), P(t["dparams"]), m, Cf,
                                                               P(t["workspace"]), nbytes, S())), \
                [In("values", _f(rng, (n, Cf), 2.0)), In("params", torch.tensor(ec.factorized_params(Cf)[1])), Out("dvalues", (n, Cf), F32),
                 Out("dparams", (Cf * 44,), F32), Scratch("workspace", nbytes)]
        if name == "bce_bwd":
            return (lambda t: L.pcgc_bce_bwd(P(t["pred"]), P(t["label"]), 0.003, 0.04, P(t["dpred"]), n, S())), \
                [In("pred", _f(rng, (n,), 2.0)), In("label", torch.from_numpy((rng.random(n) < 0.3).astype(np.float32))), Out("dpred", (n,), F32)]
        if name == "sum_log":
            nbytes = int(L.pcgc_sum_log_workspace_bytes())
            return (lambda t: L.pcgc_sum_log(P(t["p"]), n, P(t["out"]), P(t["workspace"]), nbytes, S())), \
                [In("p", torch.from_numpy(rng.uniform(1e-9, 1.0, n).astype(np.float32))), Out("out", (1,), F64), Scratch("workspace", nbytes)]
        if name == "adam_step":
            return (lambda t: L.pcgc_adam_step(P(t["param"]), P(t["grad"]), P(t["m"]), P(t["v"]), n, 1e-3, 0.9, 0.999, 1e-8, S())), \
                [InOut("param", _f(rng, (n,))), In("grad", _f(rng, (n,))), InOut("m", _f(rng, (n,), 0.1)), InOut("v", _f(rng, (n,), 0.1).abs())]
        raise KeyError(name)
    return make


for name in ("relu_bwd", "relu_bwd copy", "vrn_merge", "vrn_bwd_split", "vrn_bwd_split premasked", "vrn_bwd_split_signs", "abs_max",
             "abs_max gradient", "add_inplace", "laplace_likelihood_bwd", "factorized_likelihood_bwd C1", "factorized_likelihood_bwd C8",
             "bce_bwd", "sum_log", "adam_step"):
    for n in (1, 255, 257, 4099):
        row("%s n%d" % (name, n), _elementwise(name, n))


# ----------------------------------------------------------------------------------------------------------------------
# The voxel-grid metrics (tail.hip D1 / D2, color.hip, mesh.hip): workspaces carved by hand (pcgc_d1_*, pcgc_d2_*: sums of size_t
# terms) or by a Carver layout, a bit set whose scan "reads no bound" because it is padded to whole scan blocks.  res 51: 132 651
# cells, two scan blocks of 131 072 bits, the second one barely begun; a few hundred points in two clusters that reach the first
# and the last cell.  (tests/test_gpu_grid_range.py runs the same entry points at the top of their range.)
# ----------------------------------------------------------------------------------------------------------------------
GRID_RES = 51


def _grid_cloud(seed):
    """int32 [n,3] in a seeded order: a cluster through the last cell of the grid, a smaller one through the first"""
    rng = _rng("grid cloud", seed)
    p = np.concatenate([GRID_RES - 1 - rng.integers(0, 12, (300, 3)), rng.integers(0, 6, (40, 3)), [[0, 0, 0]], [[GRID_RES - 1] * 3]])
    p = np.unique(p, axis=0)
    return torch.from_numpy(p[rng.permutation(len(p))].astype(np.int32)), rng


def _sorted_keys(p):
    p = p.to(I64)
    return torch.sort((p[:, 0] * GRID_RES + p[:, 1]) * GRID_RES + p[:, 2])[0].contiguous()


def _grid_metric(name):
    def make():
        L, res = lib(), GRID_RES
        (a, rng), (b, _) = _grid_cloud(1), _grid_cloud(2)
        na, nb, kb = int(a.shape[0]), int(b.shape[0]), _sorted_keys(b)
        ca, cb = (torch.from_numpy(rng.integers(0, 256, (n, 3)).astype(np.uint8)) for n in (na, nb))
        if name == "d1_mse":
            nbytes = int(L.pcgc_d1_workspace_bytes(res))
            return (lambda t: L.pcgc_d1_mse(P(t["pa"]), na, P(t["pb"]), nb, res, P(t["out2"]), P(t["workspace"]), nbytes, S())), \
                [In("pa", a), In("pb", b), Out("out2", (2,), F64), Scratch("workspace", nbytes)]
        if name == "d2_transfer_normals":
            nbytes = int(L.pcgc_d2_workspace_bytes(res, nb))
            return (lambda t: L.pcgc_d2_transfer_normals(P(t["p"]), na, P(t["normals_p"]), P(t["qkeys"]), nb, res, P(t["normals_q"]),
                                                         P(t["workspace"]), nbytes, S())), \
                [In("p", a), In("normals_p", _f(rng, (na, 3))), In("qkeys", kb), Out("normals_q", (nb, 3), F32), Scratch("workspace", nbytes)]
        if name == "d2_mse":
            nbytes = int(L.pcgc_d2_workspace_bytes(res, nb))
            return (lambda t: L.pcgc_d2_mse(P(t["p"]), na, P(t["qkeys"]), nb, P(t["normals_q"]), res, P(t["out2"]), P(t["workspace"]), nbytes, S())), \
                [In("p", a), In("qkeys", kb), In("normals_q", _f(rng, (nb, 3))), Out("out2", (2,), F64), Scratch("workspace", nbytes)]
        if name == "recolor":
            nbytes = int(L.pcgc_recolor_workspace_bytes(res, na, nb))
            return (lambda t: L.pcgc_recolor(P(t["source_points"]), P(t["source_colors"]), na, P(t["target_keys"]), nb, res, P(t["target_colors"]),
                                             P(t["backward_counts"]), P(t["workspace"]), nbytes, S())), \
                [In("source_points", a), In("source_colors", ca), In("target_keys", kb), Out("target_colors", (nb, 3), U8),
                 Out("backward_counts", (nb,), I32), Scratch("workspace", nbytes)]
        if name == "color_mse":
            nbytes = int(L.pcgc_color_mse_workspace_bytes(res, nb))
            return (lambda t: L.pcgc_color_mse(P(t["points_a"]), P(t["colors_a"]), na, P(t["points_b"]), P(t["colors_b"]), nb, res, P(t["out3"]),
                                               P(t["workspace"]), nbytes, S())), \
                [In("points_a", a), In("colors_a", ca), In("points_b", b), In("colors_b", cb), Out("out3", (3,), F64), Scratch("workspace", nbytes)]
        if name == "mesh_voxelize":                            # resolution 50: the grid of resolution + 1 = 51 cells per axis
            n = 500
            pts = torch.from_numpy(rng.uniform(-3.0, 4.0, (n, 3)))
            nbytes = int(L.pcgc_mesh_voxelize_workspace_bytes(res - 1))
            return (lambda t: L.pcgc_mesh_voxelize(P(t["points"]), n, res - 1, P(t["out"]), n, P(t["n_out"]), P(t["workspace"]), nbytes, S())), \
                [In("points", pts), Out("out", (n, 3), I32), Out("n_out", (1,), I64), Scratch("workspace", nbytes)]
        if name == "estimate_normals":
            nbytes = int(L.pcgc_normals_workspace_bytes(res, na, 10.0))
            return (lambda t: L.pcgc_estimate_normals(P(t["points"]), na, res, 10.0, 20, P(t["normals"]), P(t["cov"]), P(t["n_neighbours"]),
                                                      P(t["workspace"]), nbytes, S())), \
                [In("points", a), Out("normals", (na, 3), F32), Out("cov", (na, 6), I64), Out("n_neighbours", (na,), I32),
                 Scratch("workspace", nbytes)]
        raise KeyError(name)
    return make


GRID_METRICS = ("d1_mse", "d2_transfer_normals", "d2_mse", "recolor", "color_mse", "mesh_voxelize", "estimate_normals")
for name in GRID_METRICS:
    row("%s res%d" % (name, GRID_RES), _grid_metric(name))


# ----------------------------------------------------------------------------------------------------------------------
def _with_env(monkeypatch, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)


@pytest.mark.parametrize("name,env,make", ROWS)
def test_operands_in_arenas(name, env, make, monkeypatch):
    """The same bytes on plain allocations and in arenas under three pad fills; pads, inputs and scratch surroundings untouched;
    return code 0 (tests/_arena.py)."""
    _with_env(monkeypatch, env)
    call, operands = make()
    _arena.run(Case(name, call, operands), "cuda")


@pytest.mark.parametrize("name,env,make", EMPTY_ROWS)
def test_empty_calls_touch_nothing(name, env, make, monkeypatch):
    """pcgc.h: empty inputs are valid no-ops that return 0 without touching any pointer."""
    _with_env(monkeypatch, env)
    call, operands = make()
    _arena.run_noop(Case(name, call, operands), "cuda")


def test_the_table_names_every_hot_path_entry_point():
    """A later entry point of these families is a row of the table: the ones the issue lists are all there."""
    names = " ".join(p.values[0] for p in ROWS)
    for fn in ("conv3d_fwd", "vrn_fwd", "net_forward analysis", "net_forward synthesis", "net_forward hyper encoder", "net_forward hyper decoder",
               "rowocc", "round_minmax ", "round_minmax_i16", "symbols_to_values ", "symbols_to_values_seg", "laplace_likelihood ",
               "factorized_likelihood ", "factorized_pmf", "laplace_cdf", "topk_threshold", "voxelize_points", "bce_sums", "train_loss_sums",
               "conv3d_bwd_data", "conv3d_bwd_weight", "vrn_fwd_train ", "vrn_fwd_train_signs", "vrn_fwd_train_q4", "vrn_bwd_input ",
               "vrn_bwd_input_q4", "vrn_bwd_tail ", "vrn_bwd_tail_split ", "vrn_bwd_tail_split_q4", "relu_bwd", "vrn_merge", "vrn_bwd_split ",
               "vrn_bwd_split_signs", "abs_max", "add_inplace", "laplace_likelihood_bwd", "factorized_likelihood_bwd", "bce_bwd", "sum_log",
               "adam_step"):
        assert fn in names, fn


def test_the_table_names_the_voxel_grid_metrics():
    names = [p.values[0] for p in ROWS]
    for fn in GRID_METRICS:
        assert "%s res%d" % (fn, GRID_RES) in names, fn


# ----------------------------------------------------------------------------------------------------------------------
# Top-k edges against the oracle's rule (oracle.points.adaptive_threshold / select_voxels), mask and threshold bit for bit.
# ----------------------------------------------------------------------------------------------------------------------
def _topk_cubes(cs):
    """name -> (cube [vox] float32, k) at cube size cs."""
    vox = cs ** 3
    rng = _rng("topk edges", cs)
    base = (rng.standard_normal(vox) * 3.0).astype(np.float32)
    few = np.where(base > -2.0, np.float32(-2.0) - np.abs(base), base).astype(np.float32)       # everything <= -2.0 ...
    few[rng.choice(vox, 5, replace=False)] = np.float32([0.5, 1.5, -1.0, 3.0, -1.999])           # ... but five candidates
    negative = (-np.abs(base) - np.float32(0.001)).astype(np.float32)
    n_cand = int((base > -2.0).sum())
    zeros = base.copy()
    zeros[np.abs(zeros) < 1.0] = 0.0
    zi = np.flatnonzero(zeros == 0.0)
    zeros[zi[::2]] = np.float32(-0.0)                                                           # both zeros, half each
    k_zero = int((zeros > 0).sum()) + 3                                                        # the threshold lands among the zeros
    assert (zeros == 0).sum() > 6 and np.signbit(zeros[zeros == 0]).any() and not np.signbit(zeros[zeros == 0]).all()
    ties = np.round(base).astype(np.float32)                                                   # a dozen distinct values: heavy ties
    k_ties = int((ties > 1.0).sum()) + 2                                                       # ... and the threshold is one of them (1.0)
    return {
        "fewer than k candidates": (few, 9),
        "all negative": (negative, max(1, vox // 50)),
        "all negative, below -2": ((negative - np.float32(2.0)).astype(np.float32), max(1, vox // 50)),
        "k == 0": (base, 0),
        "k == vox": (base, vox),
        "k == candidates": (base, n_cand),
        "k == candidates + 1": (base, n_cand + 1),
        "both zeros at the threshold": (zeros, k_zero),
        "heavy ties": (ties, k_ties),
    }


@pytest.mark.parametrize("cs", [64, 16, 8])
def test_topk_edges_match_the_oracle(cs):
    """The branches of topk_kernel (tail.hip) the golden vectors never take: all voxels as candidates, the inverted-key half of
    the radix (a threshold below zero), k = 0, k = vox, k = number of candidates, -0.0 and +0.0 at the threshold, heavy ties, and
    cubes smaller than the workgroup (8^3 = 512 < 1024 threads).  One launch per cube size holds every case as a cube of its own."""
    cases = _topk_cubes(cs)
    vox = cs ** 3
    x = np.stack([c for c, _ in cases.values()])
    k = np.array([kk for _, kk in cases.values()], np.int32)
    B = len(cases)
    xd, kd = torch.from_numpy(x).cuda(), torch.from_numpy(k).cuda()
    thr = torch.empty(B, dtype=F32, device="cuda")
    mask = torch.full((B, vox), 9, dtype=U8, device="cuda")
    nbytes = int(lib().pcgc_topk_workspace_bytes(B, vox))
    ws = torch.empty(max(nbytes, 1), dtype=U8, device="cuda")
    _lib.check(lib().pcgc_topk_threshold(P(xd), P(kd), B, vox, 0, 0.0, P(thr), P(mask), P(ws), nbytes, S()), "pcgc_topk_threshold")
    thr, mask = thr.cpu().numpy(), mask.cpu().numpy()
    for b, (name, (cube, kk)) in enumerate(cases.items()):
        want = opoints.adaptive_threshold(cube, kk)
        want_mask = opoints.select_voxels(cube[None], [kk])[0].astype(np.uint8)
        if name == "both zeros at the threshold":
            assert want == 0.0 and thr[b] == want, (name, thr[b], want)               # equal as floats: either zero selects the same voxels
        else:
            assert thr[b].view(np.uint32) == np.float32(want).view(np.uint32), (name, thr[b], want)
        assert np.array_equal(mask[b], want_mask), (name, int((mask[b] != want_mask).sum()))
        if name in ("fewer than k candidates", "all negative, below -2"):
            assert want <= -2.0, name
        if name.startswith("all negative"):
            assert want < 0 and 0 < want_mask.sum() < vox, name
    # k > vox: an IndexError in the reference, a documented clamp here (tail.hip: rank 0, so every voxel is selected)
    with pytest.raises(IndexError):
        opoints.adaptive_threshold(x[0], vox + 1)
    kd = torch.full((B,), vox + 1, dtype=I32, device="cuda")
    thr2 = torch.empty(B, dtype=F32, device="cuda")
    mask2 = torch.full((B, vox), 9, dtype=U8, device="cuda")
    _lib.check(lib().pcgc_topk_threshold(P(xd), P(kd), B, vox, 0, 0.0, P(thr2), P(mask2), P(ws), nbytes, S()), "pcgc_topk_threshold")
    assert np.array_equal(thr2.cpu().numpy(), x.min(1)) and bool((mask2 == 1).all())
