"""Seeded voxel clouds (int32 points, uint8 colours) that the colour tests and the exact D1 / D2 tests share."""
import numpy as np


def dense(seed, res, n):
    """n random cells of the res^3 grid without repeats, in random order, with a random colour each"""
    rng = np.random.default_rng(seed)
    p = np.unique(rng.integers(0, res, (n, 3)), axis=0).astype(np.int32)
    p = p[rng.permutation(len(p))]
    return p, rng.integers(0, 256, (len(p), 3)).astype(np.uint8)


def faces(seed, res, n):
    """a cloud that touches all six faces of the grid: a coarse lattice that includes the eight corners, each point moved by up
    to two cells (clipped, so the faces keep points), plus n random points near lattice points — the two clouds of a pair stay
    within a few cells of each other, which keeps the shell search short at res 1024"""
    rng = np.random.default_rng(seed)
    axis = np.unique(np.r_[0:res:max(8, res // 8), res - 1])
    lattice = np.stack(np.meshgrid(axis, axis, axis, indexing="ij"), -1).reshape(-1, 3)
    corners = lattice[np.all((lattice == 0) | (lattice == res - 1), 1)]
    moved = lattice + rng.integers(-2, 3, lattice.shape)
    extra = lattice[rng.integers(0, len(lattice), n)] + rng.integers(-3, 4, (n, 3))
    p = np.unique(np.clip(np.concatenate([corners, moved, extra]), 0, res - 1), axis=0).astype(np.int32)
    assert p.min(0).tolist() == [0, 0, 0] and p.max(0).tolist() == [res - 1] * 3
    p = p[rng.permutation(len(p))]
    return p, rng.integers(0, 256, (len(p), 3)).astype(np.uint8)
