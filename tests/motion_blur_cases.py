"""What the ff_motion_blur tests on the host and on the GPU share: the image sizes, the seeded inputs and the bitwise comparison."""
import functools

import numpy as np

import motion_blur_ref as R

SIZES = [(1, 1), (1, 7), (5, 3), (17, 9), (33, 31), (64, 64), (101, 67)]  # (w, h); (33, 31) with k = 16: 3 x 2 tiles, partial on both axes


@functools.lru_cache(maxsize=None)
def inputs(w, h, seed=0):
    """Log-uniform radiance, motion of up to +-40 px with a share of exact zeros, depths with a share of misses (0)."""
    rng = np.random.default_rng(7919 * w + 31 * h + seed)
    rad = np.exp2(rng.uniform(-8.0, 4.0, (h, w, 3))).astype(np.float32)
    motion = rng.uniform(-40.0, 40.0, (h, w, 2)).astype(np.float32)
    motion[rng.random((h, w)) < 0.3] = 0.0
    depth = rng.uniform(0.5, 6.0, (h, w)).astype(np.float32)
    depth[rng.random((h, w)) < 0.2] = 0.0
    for a in (rad, motion, depth):
        a.setflags(write=False)
    return rad, motion, depth


def params_of(p):
    return dict(shutter=p.shutter, max_radius=p.max_radius, samples=p.samples, depth_extent=p.depth_extent)


def assert_same(got, want):
    (g8, g), (w8, w) = got, want
    assert np.array_equal(R.bits(g), R.bits(w)), f"{(R.bits(g) != R.bits(w)).sum()} radiance values differ"
    assert np.array_equal(g8, w8), f"{(g8 != w8).sum()} bytes differ"
