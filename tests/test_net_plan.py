"""The workspace plan of pcgc_net_forward (pcgcv1_amd/csrc/net_plan.h) on the CPU: tests/net_plan_check.cpp is a stand-alone
program that includes only that header."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def test_net_plan_regions_views_and_size(tmp_path):
    """Every combination of the four nets, 13 batch sizes, skip modes 0-3 with and without empty-cube responses and six chunk
    plans: regions aligned, ascending, disjoint and ending at `total`; every chunk's view of every table inside its region
    and below the next chunk's; the mode-3 chunk within kSegMaxChunk; the workspace no larger than the hand-written formula
    the plan replaced (restated in the checker as the oracle), and smaller by the removed slack of at most 1 280 bytes only."""
    exe = str(tmp_path / "net_plan_check")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(HERE, "net_plan_check.cpp"), "-o", exe],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stdout + build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(run.stdout)
    assert run.returncode == 0, run.stdout + run.stderr
    assert " plans checked, 0 failures" in run.stdout
