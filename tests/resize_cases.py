"""What the ff_resize tests on the host and on the GPU share: the size pairs, the kernels' tiles and the sizes around them, the seeded
images, the planted non-finite samples, the restatement fed the library's tables, and the bitwise comparison.

Every image is a noisy ramp with HDR spikes up to 1e6 and a few -0.  The horizontal kernel works on tiles of TILE_X = 64 output
columns by ROWS_H = 4 input rows (ROWS_H_SMALL = 2 where a tile's input span and weights would not fit the LDS: a Lanczos-3
reduction beyond 13 : 1), the vertical kernel on tiles of 64 columns by ROWS_V = 16 output rows, a wave on four of them."""
import functools

import numpy as np

import resize_ref as R
from gpupathtracer_amd import lib

F = np.float32
FILTERS = R.FILTERS
FILTER_NAMES = {R.BOX: "box", R.TRIANGLE: "triangle", R.MITCHELL: "mitchell", R.LANCZOS3: "lanczos3"}
FLAG_SETTINGS = (R.ANTI_RING, 0)
# ((in_w, in_h), (out_w, out_h)): the 1-pixel image both ways, both limits in both axes at once, odd ratios, one axis up and the
# other down, an equal axis
PAIRS = [((1, 1), (1, 1)), ((1, 1), (16, 16)), ((16, 16), (1, 1)), ((37, 23), (13, 7)), ((100, 3), (33, 5)), ((160, 32), (10, 2)),
         ((7, 5), (112, 80)), ((65, 9), (33, 9)), ((3, 2), (2, 3))]
# the ratios the tables are checked on, (n, N)
RATIOS = [(1, 16), (16, 1), (37, 13), (100, 33), (65, 33), (1920, 1280), (13, 37), (64, 16), (64, 32), (5, 5), (1040, 65), (3, 2), (2, 3)]

TILE_X, ROWS_H, ROWS_H_SMALL, ROWS_V = 64, 4, 2, 16
# sizes around the tiles at the non-integer ratio 1.5 (and 2 / 3), so that a tile's input span starts off a tile boundary: output
# widths 63, 64, 65 (both kernels), input heights 3, 4, 5 (the horizontal kernel's rows), output heights 15, 16, 17 (the vertical
# kernel's rows; 3, 4, 5 for its waves)
TILE_PAIRS = [((95, 23), (63, 15)), ((96, 24), (64, 16)), ((98, 26), (65, 17)), ((95, 3), (63, 3)), ((96, 4), (64, 4)), ((98, 5), (65, 5)),
              ((42, 10), (63, 15)), ((43, 11), (64, 16)), ((44, 12), (65, 17))]
# the two limits: 16 : 1 under LANCZOS3 has T = 96 and takes the horizontal kernel's small tile, more than one tile each way
LIMIT_DOWN = ((1040, 272), (65, 17))
LIMIT_UP = ((5, 3), (80, 48))
BIG = ((320, 180), (213, 120))
# non-finite samples beside the seams: 150 x 40 -> 100 x 27 has the horizontal kernel's column seam 63 | 64 at input columns 94 .. 96,
# its row seam at input rows 3 | 4, the vertical kernel's row seam 15 | 16 at input rows 23 | 24 and its wave seam 3 | 4 at rows 5 | 6
SEAM_PAIR = ((150, 40), (100, 27))
SEAM_PLANTS = {(3, 94): np.nan, (4, 96): np.inf, (23, 95): -np.inf, (24, 97): np.nan, (5, 20): np.inf, (6, 21): np.nan, (0, 0): -np.inf,
               (39, 149): np.nan, (15, 63): np.inf, (16, 64): np.nan}


@functools.lru_cache(maxsize=None)
def inputs(w, h, seed=0):
    """The finite radiance image [H,W,3] of this size, read-only."""
    rng = np.random.default_rng(7919 * w + 31 * h + seed)
    y, x = np.mgrid[0:h, 0:w]
    base = 0.05 + 1.0 * x / max(w, 1) + 0.45 * y / max(h, 1)
    rad = base[..., None] * np.array([1.0, 0.8, 0.6]) * rng.uniform(0.7, 1.3, (h, w, 3))
    wild = rng.random((h, w)) < 0.03
    rad[wild] *= np.power(10.0, rng.uniform(1.0, 6.0, (int(wild.sum()), 1)))
    rad = np.minimum(rad, 1.0e6).astype(F)
    rad[rng.random((h, w, 3)) < 0.01] = F(-0.0)
    rad.setflags(write=False)
    return rad


def planted(w, h, plants, zero=False):
    """inputs(w, h) with one channel after the other of the given (y, x) set to the given value - or, zero=True, to +0."""
    rad = np.array(inputs(w, h))
    for i, ((y, x), value) in enumerate(plants.items()):
        rad[y, x, i % 3] = 0.0 if zero else value
    return rad


def named_outputs(in_size, out_size, plants, filter):
    """[H', W'] bool: the outputs whose taps name a planted sample, through the library's tables."""
    (w, h), (ow, oh) = in_size, out_size
    fx, wx = lib.resize_weights(w, ow, filter)
    fy, wy = lib.resize_weights(h, oh, filter)
    hit = np.zeros((oh, ow), bool)
    for y, x in plants:
        cols = (np.clip(fx[:, None] + np.arange(wx.shape[1])[None, :], 0, w - 1) == x).any(axis=1)
        rows = (np.clip(fy[:, None] + np.arange(wy.shape[1])[None, :], 0, h - 1) == y).any(axis=1)
        hit |= rows[:, None] & cols[None, :]
    return hit


def reference(rad, out_size, p):
    """The restatement fed the library's tables."""
    h, w = rad.shape[:2]
    return R.resize(rad, lib.resize_weights(w, out_size[0], p.filter), lib.resize_weights(h, out_size[1], p.filter), p.flags)


def all_params():
    return [lib.resize_params(filter=f, flags=flags) for f in FILTERS for flags in FLAG_SETTINGS]


def pair_id(pair):
    (w, h), (ow, oh) = pair
    return f"{w}x{h}-{ow}x{oh}"


def assert_same(got, want):
    """rgb8 and the radiance's bits."""
    (g8, g), (w8, w) = got[:2], want[:2]
    if g is not None and w is not None:
        assert g.shape == w.shape and np.array_equal(R.bits(g), R.bits(w)), f"{(R.bits(g) != R.bits(w)).sum()} radiance values differ"
    if g8 is not None and w8 is not None:
        assert g8.shape == w8.shape and np.array_equal(g8, w8), f"{(g8 != w8).sum()} bytes differ"
