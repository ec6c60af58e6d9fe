"""Generate tests/golden/pc_error_color.npz by RUNNING the reference's prebuilt pc_error with --color=1.

Run in the build container only (needs /root/reference; the GPU box never has it):
    python tools/make_color_golden.py

Writes seeded coloured clouds as ASCII ply (x y z red green blue), runs myutils/pc_error_d -a A -b B --color=1 and
stores the clouds, their colours and the printed c[i] figures.  The fixture is data (arrays and numbers), never
reference source text.  Cases: two random dense grids (most nearest-neighbour sets hold several points), one
codec-like pair (a surface cloud and a copy with points dropped and jittered, as in pc_error_d2.npz) and hand-made ties.
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import seeded_cloud                          # noqa: E402

REF = "/root/reference"
OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")
KEYS = ["c[%d],    %s" % (i, d) for d in "12F" for i in range(3)] + ["c[%d],PSNR%s" % (i, d) for d in "12F" for i in range(3)]


def write_ply(fn, pts, colors):
    with open(fn, "w") as f:
        f.write("ply\nformat ascii 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n"
                "property uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n" % len(pts))
        for p, c in zip(pts, colors):
            f.write("%d %d %d %d %d %d\n" % (p[0], p[1], p[2], c[0], c[1], c[2]))


def dense(seed, res, n):
    rng = np.random.default_rng(seed)
    p = np.unique(rng.integers(0, res, (n, 3)), axis=0).astype(np.int32)
    p = p[rng.permutation(len(p))]
    return p, rng.integers(0, 256, (len(p), 3)).astype(np.uint8)


def textured(points, res, rng):
    """a smooth colour field over the positions plus noise, like a scanned texture"""
    t = points.astype(np.float64) / res
    c = np.stack([128 + 100 * np.sin(7 * t[:, 0] + 3 * t[:, 1]), 128 + 100 * np.cos(5 * t[:, 1] - 2 * t[:, 2]),
                  255 * t[:, 2]], -1) + rng.normal(0, 12, (len(points), 3))
    return np.clip(np.rint(c), 0, 255).astype(np.uint8)


def main():
    os.makedirs(OUT, exist_ok=True)
    tmp = tempfile.mkdtemp(prefix="golden_color_")
    cases = []
    for sa, sb, res, na, nb in [(61, 62, 12, 600, 500), (63, 64, 16, 2200, 1500)]:
        a, ca = dense(sa, res, na)
        b, cb = dense(sb, res, nb)
        cases.append((a, ca, b, cb, res))
    res = 128
    a = seeded_cloud(71, res, 3000)
    rng = np.random.default_rng(171)
    ca = textured(a, res, rng)
    keep = rng.random(len(a)) > 0.15
    b = a[keep].copy()
    b += rng.integers(-1, 2, b.shape).astype(np.int32) * (rng.random(b.shape) < 0.3)
    b, first = np.unique(np.clip(b, 0, res - 1), axis=0, return_index=True)
    cb = np.clip(ca[keep][first].astype(np.int64) + rng.integers(-6, 7, (len(b), 3)), 0, 255).astype(np.uint8)
    cases.append((a, ca, b.astype(np.int32), cb, res))
    # hand-made ties: two, four and six nearest points whose means end in .5 (round half up), a lone pair, an identity
    cases.append((np.array([[1, 1, 1], [5, 5, 5], [9, 1, 1]], np.int32), np.array([[10, 200, 30], [255, 0, 128], [1, 2, 3]], np.uint8),
                  np.array([[0, 1, 1], [2, 1, 1], [5, 4, 5], [5, 6, 5], [4, 5, 5], [6, 5, 5], [5, 5, 4], [5, 5, 6], [9, 1, 3]], np.int32),
                  np.array([[0, 0, 0], [1, 255, 3], [10, 20, 30], [11, 20, 31], [10, 21, 30], [12, 20, 33], [10, 20, 30], [10, 25, 30],
                            [250, 251, 252]], np.uint8), 16))
    cases.append((np.array([[0, 0, 0], [0, 0, 3]], np.int32), np.array([[255, 255, 255], [0, 0, 0]], np.uint8),
                  np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1], [0, 0, 2]], np.int32),
                  np.array([[1, 0, 0], [2, 0, 255], [0, 1, 0], [128, 127, 126]], np.uint8), 16))
    cases.append((cases[0][0], cases[0][1], cases[0][0][::-1].copy(), cases[0][1][::-1].copy(), 12))
    out = {"keys": np.array(KEYS), "n_cases": np.array(len(cases))}
    for i, (a, ca, b, cb, res) in enumerate(cases):
        fa, fb = os.path.join(tmp, "a%d.ply" % i), os.path.join(tmp, "b%d.ply" % i)
        write_ply(fa, a, ca)
        write_ply(fb, b, cb)
        text = subprocess.run([os.path.join(REF, "myutils", "pc_error_d"), "-a", fa, "-b", fb, "--color=1", "--hausdorff=1",
                               "--resolution=%d" % (res - 1)], capture_output=True, text=True).stdout
        vals = {}
        for line in text.splitlines():
            for key in KEYS:
                if line.strip().startswith(key):              # (the " h.c[i]" lines do not start with c[)
                    vals[key] = float(line.split(":")[-1])
        assert sorted(vals) == sorted(KEYS), text
        out["a%d" % i], out["ca%d" % i], out["b%d" % i], out["cb%d" % i], out["res%d" % i] = a, ca, b, cb, np.array(res)
        out["vals%d" % i] = np.array([vals[k] for k in KEYS])
        print("pc_error colour", i, len(a), len(b), vals)
    path = os.path.join(OUT, "pc_error_color.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
