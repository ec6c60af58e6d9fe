"""The weight-gradient dispatch (pcgcv1_amd/csrc/dw_plan.h) on the CPU: tests/dw_plan_check.cpp is a stand-alone program that
includes only that header; the layer shapes come from models/spec.py, the layouts from Trainer._q4_flags."""
import os
import subprocess

from pcgcv1_amd.models import spec
from pcgcv1_amd.train_hyper import Trainer

HERE = os.path.dirname(os.path.abspath(__file__))


def _layer_records():
    """One line per layer, net and cube size (16, 32, 64): label kind cin cout k stride D-of-the-layer-input x_q4 y_q4, in NDHWC
    and, at cube size 64, also in the layouts the Q4 training step gives the layer; a `pair` line for conv1_1 + conv2_1 of
    every block (the two layers the step hands to launch_conv_dw_pair)."""
    first = {"analysis_transform": 1, "synthesis_transform": 4, "hyper_encoder": 4, "hyper_decoder": 8}
    tables = [(name, fn, first[name], True) for name, fn in spec.NETS.items()]
    tables += [("simple_" + name, fn, {"analysis_transform": 1, "synthesis_transform": 8}[name], False) for name, fn in spec.SIMPLE_NETS.items()]
    lines = []
    for cube in (16, 32, 64):
        for net, fn, div, voxception in tables:
            D = cube // div
            for l in fn():
                layouts = [(0, 0)]
                if cube == 64 and voxception and Trainer._q4_flags(net, l) != (0, 0):
                    layouts.append(Trainer._q4_flags(net, l))
                for xq, yq in layouts:
                    label = "%s/%s@%d" % (net, l.name, cube)
                    lines.append("%s %s %d %d %d %d %d %d %d" % (label, l.kind, l.cin, l.cout, l.k, l.stride, D, xq, yq))
                    if l.name.endswith("/conv1_1"):
                        lines.append("%s+conv2_1 pair %d %d 3 1 %d %d 0" % (label, l.cin, l.cout, D, xq))
                D = 2 * D if l.kind == "tconv" else D // l.stride
    return lines


def test_dw_dispatch_matches_the_ladder_it_replaced(tmp_path):
    """Over Cin, Cout in {1, 2, 4, 8, 16, 32, 48, 64}, ksize 1 / 3 / 5, D in {4 .. 64}, B in {1, 2, 8, 24} and the four Q4 flag
    combinations (and the stride-2 pair with fine_q4, and conv_dw_pair_supported): the same kernel, groups, channel chunks,
    batchable flag and refusal as the ladder of launch_conv_dw_tile / _s2 before the table (restated in the checker), except on
    the printed exceptions, each "a deleted instantiation -> the generic kernel"; no layer of any net at cube sizes 16 / 32 / 64
    among them; every enum value chosen for some input; every partial buffer at least groups x (weights + bias sums)."""
    records = _layer_records()
    assert len(records) > 250
    layers = tmp_path / "layers.txt"
    layers.write_text("\n".join(records) + "\n")
    exe = str(tmp_path / "dw_plan_check")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(HERE, "dw_plan_check.cpp"), "-o", exe],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stdout + build.stderr
    run = subprocess.run([exe, str(layers)], capture_output=True, text=True, timeout=120)
    print(run.stdout)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "%d layer records, 0 failures" % len(records) in run.stdout
    # the shapes that lost their tuned kernel: exactly the families DESIGN.md lists
    exceptions = sorted(line.split(":")[0].replace("EXCEPTION stride 1 ", "").strip() for line in run.stdout.splitlines() if "EXCEPTION" in line)
    assert exceptions == sorted(["k=3 8 -> 32", "k=3 8 -> 4", "k=3 4 -> 16", "k=3 32 -> 1", "k=3 48 -> 1", "k=3 64 -> 1",
                                 "k=1 32 -> 4", "k=1 48 -> 4", "k=1 64 -> 4"])
