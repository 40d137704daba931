"""What the ff_despeckle tests on the host and on the GPU share: the image sizes, the seeded inputs with their planted spikes, the
parameter grid and the bitwise comparison.

The kernel works on tiles of 32 x 8 pixels with an apron of r pixels: the planted spikes at SEAMS lie within r pixels of the seams
x = 32 and y = 8, on each side, in pairs whose other half lies across the seam, so that the neighbour across the seam decides whether
a spike survives."""
import functools

import numpy as np

import despeckle_ref as R

F = np.float32
DIFFUSE, MIRROR, EMITTER = 1, 2, 0
# (w, h): image edges inside, on and just past a tile edge in both axes
SIZES = [(1, 1), (1, 7), (7, 1), (15, 17), (16, 16), (17, 15), (31, 33), (33, 9), (101, 67)]
RADII, RANKS = (1, 2, 3), (1, 2, 3, 4)
PLANT_SIZE = (101, 67)  # the size of the planted-spike tests (any size from 48 x 24 on carries the spikes)

# planted spikes as (y, x) lists; every group keeps 7 pixels from the next, from the geometry borders and from the image edge
SINGLES = [(20, 8), (20, 20), (36, 12), (44, 76), (28, 88)]                # factors x10 .. x1e6
PAIRS = [[(28, 8), (28, 9)], [(36, 24), (37, 24)], [(44, 88), (44, 89)]]   # adjacent: side by side and one above the other
BLOCK = [(28, 20), (28, 21), (29, 20), (29, 21)]                           # 2 x 2
# across the seams x = 32 (columns 31 | 32) and y = 8 (rows 7 | 8), 1, 2 and 3 pixels apart: each pair's halves see each other
# only through the apron, and only from the radius of their distance on
SEAMS = [[(20, 31), (20, 32)], [(7, 8), (8, 8)], [(36, 30), (36, 32)], [(6, 20), (8, 20)], [(44, 30), (44, 33)], [(6, 28), (9, 28)],
         [(7, 63), (8, 64)]]  # (the last: diagonally across the corner of four tiles at x = 64, y = 8)
FACTORS = [10.0, 1.0e2, 1.0e3, 1.0e4, 1.0e5, 1.0e6]


def planted(w, h):
    """{(y, x): factor} of the spikes an image of this size carries (none below 48 x 24)."""
    if w < 48 or h < 24:
        return {}
    spikes = {}
    for i, yx in enumerate(SINGLES):
        spikes[yx] = FACTORS[i % len(FACTORS)] if i else FACTORS[-1]
    for i, group in enumerate(PAIRS + SEAMS):
        for yx in group:
            spikes[yx] = FACTORS[(i + 2) % len(FACTORS)]
    for yx in BLOCK:
        spikes[yx] = 1.0e3
    return {(y, x): f for (y, x), f in spikes.items() if y < h - 3 and x < w - 3}


def regions(w, h):
    """The ids plane [H,W,3] {geometry, triangle, bxdf}: three geometries side by side (the third a mirror), a band of misses along
    the bottom, an emitter patch in the top right corner and a strip of a fourth geometry one pixel wide and three long."""
    ids = np.zeros((h, w, 3), np.int32)
    x = np.arange(w)[None, :]
    ids[..., 0] = np.where(3 * x < w, 0, np.where(3 * x < 2 * w, 1, 2))
    ids[..., 1] = (np.arange(h)[:, None] // 2 + x // 3) % 7
    ids[..., 2] = np.where(ids[..., 0] == 2, MIRROR, DIFFUSE)
    if h >= 4:
        ids[h - max(1, h // 8):] = (-1, -1, -1)
    if w >= 8 and h >= 4:
        ids[:h // 8 + 1, w - w // 8 - 1:] = (4, 0, EMITTER)
    if w >= 5 and h >= 5:
        ids[1:4, w // 2] = (3, 0, DIFFUSE)
    return ids


def ramp(w, h):
    """A smooth positive ramp: 0.5 .. 1 over the image, tinted per channel.  Between pixels 3 apart it changes by less than
    3 (0.3 / w + 0.2 / h) of at least 0.5: far from the factor 2 of the default threshold for every size here with more than
    a few pixels, and the tests assert on the reference that no unplanted pixel of the ramp is clamped."""
    y, x = np.mgrid[0:h, 0:w]
    base = 0.5 + 0.3 * x / max(w, 1) + 0.2 * y / max(h, 1)
    return (base[..., None] * np.array([1.0, 0.8, 0.6])).astype(F)


@functools.lru_cache(maxsize=None)
def inputs(w, h, seed=0, noise=True):
    """(radiance, albedo, ids), read-only.  noise=True: the ramp under +-30 % of noise and a sprinkle of random spikes beside the
    planted ones, a random albedo with zero and negative channels in places.  noise=False: the ramp itself with the planted spikes
    alone over an albedo that is constant per geometry."""
    rng = np.random.default_rng(7919 * w + 31 * h + seed)
    ids = regions(w, h)
    rad = ramp(w, h)
    if noise:
        rad = (rad * rng.uniform(0.7, 1.3, (h, w, 3))).astype(F)
        wild = rng.random((h, w)) < 0.03
        rad[wild] = (rad[wild] * np.power(10.0, rng.uniform(1.0, 6.0, (int(wild.sum()), 1)))).astype(F)
        albedo = rng.uniform(0.2, 0.9, (h, w, 3)).astype(F)
        albedo[rng.random((h, w, 3)) < 0.03] = 0.0
        albedo[rng.random((h, w, 3)) < 0.02] = -0.5
    else:
        albedo = np.empty((h, w, 3), F)
        albedo[:] = (0.5, 0.25, 0.75)
        albedo[ids[..., 0] == 1] = (0.8, 0.8, 0.2)
    for (y, x), f in planted(w, h).items():
        rad[y, x] = (ramp(w, h)[y, x] * F(f)).astype(F)
    for a in (rad, albedo, ids):
        a.setflags(write=False)
    return rad, albedo, ids


def params_of(p):
    return dict(radius=p.radius, rank=p.rank, min_neighbours=p.min_neighbours, threshold=p.threshold, floor=p.floor, flags=p.flags)


def reference(rad, albedo, ids, p, **kw):
    return R.despeckle(rad, albedo, ids, **params_of(p), **kw)


def assert_same(got, want):
    """rgb8, radiance bits and the count."""
    (g8, g, gn), (w8, w, wn) = got[:3], want[:3]
    if g is not None and w is not None:
        assert np.array_equal(R.bits(g), R.bits(w)), f"{(R.bits(g) != R.bits(w)).sum()} radiance values differ"
    if g8 is not None and w8 is not None:
        assert np.array_equal(g8, w8), f"{(g8 != w8).sum()} bytes differ"
    assert gn == wn, f"clamped {gn} != {wn}"
