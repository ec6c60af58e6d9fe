"""Seeded inputs of the cube-size tests (test_gpu_cube_sizes.py, test_cube_sizes_host.py) and the CPU oracle's results on them.

The batch of a cube size cs, in this order:
  0..2  synthetic.make_cubes(seed=3, n_cubes=3, cube_size=cs, occupancy=0.03): wavy sheets across axis d, h and w
  3     an all-zero cube
  4     single voxels at (0,0,0), (cs-1,cs-1,cs-1) and (0,cs-1,0)                         (indices d, h, w)
  5     the full planes w = 0, w = cs-1, d = 0 and h = cs-1
  6     default_rng(3).random(...) < 0.3
Weights: synthetic.make_weights(seed=11, profile="dense").

RANGE_SAFE names the cubes whose rounded latents stay inside the container's |min|, |max| <= 15 at 32 and 16 (the third
sheet and the 30 % cube do not: test_cube_sizes_host.py pins both facts), i.e. the cubes the entropy stage can code.
"""
import functools

import numpy as np

from oracle import nets as onets
from pcgcv1_amd import synthetic

SHEETS, EMPTY, CORNERS, FACES, RANDOM = (0, 1, 2), 3, 4, 5, 6
N_CUBES = 7
RANGE_SAFE = (0, 1, EMPTY, CORNERS, FACES)
CKPT = "t_cube_sizes"                      # the key the GPU tests bind the weights to in checkpoint._CACHE


@functools.lru_cache(maxsize=None)
def weights():
    return synthetic.make_weights(seed=11, profile="dense")


@functools.lru_cache(maxsize=None)
def batch(cs):
    """float32 [7, cs, cs, cs, 1]; read-only (shared among the tests)."""
    x = np.zeros((N_CUBES, cs, cs, cs, 1), np.float32)
    x[:3] = synthetic.make_cubes(seed=3, n_cubes=3, cube_size=cs, occupancy=0.03)
    for d, h, w in ((0, 0, 0), (cs - 1, cs - 1, cs - 1), (0, cs - 1, 0)):
        x[CORNERS, d, h, w, 0] = 1.0
    x[FACES, :, :, 0], x[FACES, :, :, cs - 1], x[FACES, 0], x[FACES, :, cs - 1] = 1.0, 1.0, 1.0, 1.0
    x[RANDOM] = np.random.default_rng(3).random((cs, cs, cs, 1)) < 0.3
    x.setflags(write=False)
    return x


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


@functools.lru_cache(maxsize=None)
def oracle_y(cs, n):
    """The oracle's latents of the first n cubes."""
    return _frozen(onets.analysis_transform(onets.sub(weights(), "analysis_transform"), np.array(batch(cs)[:n])))


@functools.lru_cache(maxsize=None)
def oracle_z(cs, n):
    return _frozen(onets.hyper_encoder(onets.sub(weights(), "hyper_encoder"), np.array(oracle_y(cs, n))))


@functools.lru_cache(maxsize=None)
def oracle_loc_scale(cs, n):
    """The oracle's hyper decoder on rint(z), scale clamped at 1e-9 like the codec's call."""
    loc, scale = onets.hyper_decoder(onets.sub(weights(), "hyper_decoder"), np.rint(oracle_z(cs, n)))
    return _frozen(loc, np.maximum(scale, np.float32(1e-9)))


@functools.lru_cache(maxsize=None)
def oracle_x(cs, n):
    """The oracle's synthesis of rint(y)."""
    return _frozen(onets.synthesis_transform(onets.sub(weights(), "synthesis_transform"), np.rint(oracle_y(cs, n))))
