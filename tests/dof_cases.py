"""What the ff_depth_of_field tests on the host and on the GPU share: the image sizes, the seeded inputs, the camera and the bitwise
comparison."""
import functools

import numpy as np

from gpupathtracer_amd import scenes
import dof_ref as R
from motion_blur_cases import SIZES  # (w, h); (33, 31) with k = 16: 3 x 2 tiles, partial on both axes

assert SIZES == [(1, 1), (1, 7), (5, 3), (17, 9), (33, 31), (64, 64), (101, 67)]
# (max_radius, grid): the defaults, the smallest of both, every lane-group size of the pack kernel and both sides of its switch
KG = [(16, 4), (1, 1), (2, 8), (64, 2), (5, 3), (8, 4), (9, 4)]
DEFAULTS = dict(focus_distance=2.0, coc_scale=20.0)  # radii from 0 (z = 2) to beyond k = 16 (z < 0.77): in focus, blurred and clamped


def camera(w, h):
    """At the origin, looking down -z."""
    return scenes.posed_camera(w, h, position=(0.0, 0.0, 0.0), yaw=-90.0, pitch=0.0)


@functools.lru_cache(maxsize=None)
def inputs(w, h, seed=0):
    """Log-uniform radiance; positions of axial depth 0.5 .. 6 in front of camera(w, h) with a small lateral scatter, their distance
    as the depth plane; a 20 % share of misses (depth 0, position 0)."""
    rng = np.random.default_rng(104729 * w + 37 * h + seed)
    rad = np.exp2(rng.uniform(-8.0, 4.0, (h, w, 3))).astype(np.float32)
    pos = np.empty((h, w, 3), np.float32)
    pos[..., :2] = rng.uniform(-0.2, 0.2, (h, w, 2))
    pos[..., 2] = -rng.uniform(0.5, 6.0, (h, w))
    depth = np.sqrt((pos.astype(np.float64) ** 2).sum(axis=-1)).astype(np.float32)
    miss = rng.random((h, w)) < 0.2
    pos[miss] = 0.0
    depth[miss] = 0.0
    for a in (rad, pos, depth):
        a.setflags(write=False)
    return rad, pos, depth


def vec(v):
    return np.array([v.x, v.y, v.z], np.float32)


def params_of(p):
    return dict(focus_distance=p.focus_distance, coc_scale=p.coc_scale, max_radius=p.max_radius, grid=p.grid, depth_extent=p.depth_extent)


def reference(rad, pos, depth, cam, p, **kw):
    return R.depth_of_field(rad, pos, depth, vec(cam.m_position), vec(cam.m_forward), **params_of(p), **kw)


def assert_same(got, want):
    (g8, g), (w8, w) = got, want
    assert np.array_equal(R.bits(g), R.bits(w)), f"{(R.bits(g) != R.bits(w)).sum()} radiance values differ"
    assert np.array_equal(g8, w8), f"{(g8 != w8).sum()} bytes differ"
