"""No GPU: what keeps tests/test_gpu_train_dw.py honest.  (1) tests/dw_cases_check.cpp — a stand-alone program on
csrc/dw_plan.h — says which kernel every case of tests/_dw_cases.py takes and how many tiles its grid walks: every tiled
kernel of the table must be run multi-tile and uneven.  (2) The float64 reference of tests/_dw_ref.py against float64 autograd
of the oracle's convolution (oracle/train.py:_conv): padding and filter layouts of the three kinds of layer."""
import os
import subprocess

import pytest

import _dw_cases

HERE = os.path.dirname(os.path.abspath(__file__))
ONE_U = 4          # conv_dw_1x1_kernel: strides a thread requests per round (constexpr int U in train_dw.hip)


@pytest.fixture(scope="module")
def audit(tmp_path_factory):
    """[(case, kernel name, groups, chunks, tiles, voxels)] in the order of _dw_cases.CASES, and the table's kernel names."""
    tmp = tmp_path_factory.mktemp("dw_cases")
    records = tmp / "cases.txt"
    records.write_text("\n".join(_dw_cases.case_line(c) for c in _dw_cases.CASES) + "\n")
    exe = str(tmp / "dw_cases_check")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(HERE, "dw_cases_check.cpp"), "-o", exe],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stdout + build.stderr
    run = subprocess.run([exe, str(records)], capture_output=True, text=True, timeout=60)
    print(run.stdout)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "%d cases, 24 tiled kernels, 0 failures" % len(_dw_cases.CASES) in run.stdout
    rows, kernels = [], None
    for line in run.stdout.splitlines():
        parts = [p.strip() for p in line.split("|")]
        if parts[0].startswith("case "):
            assert int(parts[0].split()[1]) == len(rows)
            rows.append((_dw_cases.CASES[len(rows)], parts[1]) + tuple(int(p) for p in parts[2:]))
        elif parts[0] == "kernels:":
            kernels = parts[1:]
    assert len(rows) == len(_dw_cases.CASES) and kernels is not None and len(set(kernels)) == 24
    return rows, kernels


def test_every_tiled_kernel_runs_multi_tile_and_uneven(audit):
    """24 of 24: each kernel instantiation of csrc/dw_plan.h is chosen by a case whose tile count exceeds its workgroup count
    and is no multiple of it — some workgroups take one tile more than others.  The 1^3 register kernel also gets more than
    U strides (a second round of requests) ending inside a stride."""
    rows, kernels = audit
    covered = {}
    for case, name, groups, chunks, tiles, voxels in rows:
        if name != "generic" and tiles > groups and tiles % groups != 0:
            covered.setdefault(name, []).append(case)
    missing = [k for k in kernels if k not in covered]
    assert not missing, "no multi-tile, uneven case for: %s" % ", ".join(missing)
    assert len(covered) == 24
    for case, name, groups, chunks, tiles, voxels in rows:
        if name.startswith("conv_dw_1x1_kernel") and case in covered[name]:
            stride = groups * 256
            assert voxels > ONE_U * stride and voxels % stride != 0, (case, voxels, stride)
    # the launches with channel chunks (grid.y > 1) are among the uneven ones too
    assert any(chunks > 1 and case in covered.get(name, []) for case, name, groups, chunks, tiles, voxels in rows)
    # the whole-row kernels once with fewer tiles than workgroups: the idle workgroups' partials of zeros
    for name in ("conv_dw_mfma_4xn_kernel<4>", "conv_dw_mfma_4xn_kernel<8>"):
        assert any(n == name and tiles < groups for _, n, groups, _, tiles, _ in rows), name


def test_only_the_listed_cases_take_the_generic_kernel(audit):
    """A case that silently fell to conv_dw_partial_kernel would test nothing of train_dw.hip; the listed ones must take it,
    and one of them with a voxel count that is no multiple of its 128 chunks (a shorter last chunk)."""
    rows, _ = audit
    for case, name, groups, chunks, tiles, voxels in rows:
        assert (name == "generic") == (case in _dw_cases.GENERIC_CASES), (case, name)
    generic = [(case, voxels, groups) for case, name, groups, _, _, voxels in rows if name == "generic"]
    assert len(generic) == len(_dw_cases.GENERIC_CASES) >= 2
    assert any(case[0] == 3 and voxels % groups != 0 for case, voxels, groups in generic)
    assert any(case[0] == 5 and case[3] == 2 and voxels % groups != 0 for case, voxels, groups in generic)
    # the pair cases take the pair kernels, every other case is a single call
    for case, name, *_ in rows:
        assert (case[0] == "pair") == name.endswith("true>"), (case, name)


def test_cases_stay_small():
    """Under a million voxels and at most 64 channels per case: exact integer sums stay below 2^24 and a case takes a moment."""
    assert len(set(_dw_cases.CASES)) == len(_dw_cases.CASES)
    for case in _dw_cases.CASES:
        if case[0] == "pair":
            cin, cout, D, B = case[1:]
            fine = D
        else:
            k, cin, cout, stride, tr, D, B = case
            fine = 2 * D if tr else D
        assert B * fine ** 3 < 1_000_000 and max(cin, cout) <= 64, case
        assert 2 * B * fine ** 3 < 2 ** 24, case              # |x| <= 2, |dz| <= 1: every partial sum is an exact float32 integer


@pytest.mark.parametrize("k,cin,cout,stride,tr", [(3, 3, 5, 1, 0), (1, 3, 5, 1, 0), (3, 3, 5, 2, 0), (5, 3, 5, 2, 0), (3, 3, 5, 2, 1),
                                                  (5, 3, 5, 2, 1)])
def test_reference_conventions_match_the_oracles_autograd(k, cin, cout, stride, tr):
    """_dw_ref.dw_reference against float64 autograd of oracle/train.py:_conv at D = 8, B = 1, Cin != Cout: padding (the 'SAME'
    front padding of the stride-2 pair included), tap order and filter layout ([k, k, k, Cin, Cout]; transposed
    [k, k, k, Cout, Cin]); S2 against the same autograd on the squared operands."""
    torch = pytest.importorskip("torch")
    from oracle import train as otrain
    from _dw_ref import dw_reference
    g = torch.Generator().manual_seed(100 * k + 10 * stride + tr)
    D, B = 8, 1
    Do = 2 * D if tr else D // stride
    kshape = (k, k, k, cout, cin) if tr else (k, k, k, cin, cout)
    x = torch.randn((B, D, D, D, cin), generator=g, dtype=torch.float64)
    dz = torch.randn((B, Do, Do, Do, cout), generator=g, dtype=torch.float64)

    def autograd(xv, dzv):
        w = {"l/kernel": torch.randn(kshape, generator=g, dtype=torch.float64).requires_grad_(True),
             "l/bias": torch.zeros(cout, dtype=torch.float64, requires_grad=True)}
        y = otrain._conv(w, "l", xv.permute(0, 4, 1, 2, 3), stride=stride, tconv=bool(tr))
        assert tuple(y.shape) == (B, cout, Do, Do, Do)
        y.backward(dzv.permute(0, 4, 1, 2, 3))
        return w["l/kernel"].grad, w["l/bias"].grad

    ref = dw_reference(x, dz, k, stride, bool(tr))
    dk, db = autograd(x, dz)
    assert ref.dk.shape == dk.shape and float(dk.abs().max()) > 1
    torch.testing.assert_close(ref.dk, dk, rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(ref.db, db, rtol=1e-12, atol=1e-12)
    s2k, s2b = autograd(x * x, dz * dz)
    torch.testing.assert_close(ref.s2k, s2k, rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(ref.s2b, s2b, rtol=1e-12, atol=1e-12)
    assert ref.n == B * (D if tr else Do) ** 3 and ref.nb == B * Do ** 3
    # the float32 operands the GPU test passes give the same reference: the conversion to double is inside
    ref32 = dw_reference(x.float(), dz.float(), k, stride, bool(tr))
    torch.testing.assert_close(ref32.dk, dw_reference(x.float().double(), dz.float().double(), k, stride, bool(tr)).dk, rtol=0, atol=0)
