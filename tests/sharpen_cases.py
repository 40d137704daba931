"""What the ff_sharpen tests on the host and on the GPU share: the image sizes, the seeded images with their planted features, the
parameter grid and the bitwise comparison.

Every image is a noisy ramp with HDR spikes up to 1e6; whatever of the features below fits into it is planted on top.  The kernel
works on tiles of 32 x 8 pixels with a cross apron of one pixel: SEAM_EDGES put a step edge ON the seams x = 31 | 32 and y = 7 | 8,
and SEAM_UNUSABLE puts unusable pixels beside the seams and at the corners (32, 8) and (64, 8), in the noisy ramp, so that the pixel
across the seam is copied through exactly when the apron delivered its unusable neighbour."""
import functools

import numpy as np

import sharpen_ref as R

F = np.float32
# (w, h): the 1-pixel image, single rows and columns, image edges inside, on and just past a tile edge in both axes
SIZES = [(1, 1), (1, 7), (7, 1), (2, 2), (31, 33), (32, 8), (33, 9), (65, 17), (101, 67)]
BIG = (320, 180)
PLANT_SIZE = (101, 67)   # the smallest size here that carries every feature
STRENGTHS = (0.0, 0.25, 0.5, 1.0)
FLAG_SETTINGS = (R.NOISE_AWARE, 0)

# noise-free rectangles (y0, y1, x0, x1), half open
V_EDGE = (10, 18, 40, 56)       # a vertical step at x = 48: 0.1 | 2.0
H_EDGE = (20, 30, 40, 56)       # a horizontal step at y = 25
DIAGONAL = (32, 44, 40, 56)     # a step along x - y = 10
CHECKER = (10, 18, 60, 72)      # 0.1 and 0.9, pixel by pixel
SATURATED = (20, 30, 60, 72)    # a noisy red, green and blue 0 all round
BLACK = (32, 44, 60, 72)        # black, with one lit pixel in it
ISOLUMINANT = (46, 60, 44, 56)  # pixels that differ in a blue too small to reach their luminance: L is constant, t is not
SEAM_EDGES = [(46, 60, 24, 40, "x", 32), (2, 13, 2, 14, "y", 8)]  # a vertical step ON x = 31 | 32 and a horizontal one ON y = 7 | 8
LIT = (38, 66)                  # the lit pixel of BLACK
# (y, x) -> the pixel planted there.  The first four kinds are unusable; the last three are usable and take part
UNUSABLE = {(36, 10): (np.nan, 0.5, 0.25), (36, 16): (np.inf, 1.0, 1.0), (40, 10): (0.5, -0.25, 0.5), (44, 10): (1.0e7, 1.0, 1.0),
            (36, 22): (1.0, -np.inf, np.nan)}
USABLE_ODDITIES = {(40, 16): (-0.0, 0.5, 0.25), (40, 22): (-0.0, -0.0, -0.0), (44, 16): (8388608.0, 2.0, 1.0)}
# unusable pixels beside the seams: left and right of x = 31 | 32, above and below y = 7 | 8, at the corners (32, 8) and (64, 8)
SEAM_UNUSABLE = [(22, 31), (26, 32), (7, 20), (8, 26), (8, 32), (7, 63)]
EDGE_LEVELS = (0.1, 2.0)


def fits(rect, w, h):
    return rect[1] <= h and rect[3] <= w


def _noisy_ramp(w, h, rng):
    y, x = np.mgrid[0:h, 0:w]
    base = 0.05 + 1.0 * x / max(w, 1) + 0.45 * y / max(h, 1)
    rad = base[..., None] * np.array([1.0, 0.8, 0.6]) * rng.uniform(0.7, 1.3, (h, w, 3))
    wild = rng.random((h, w)) < 0.03
    rad[wild] *= np.power(10.0, rng.uniform(1.0, 6.0, (int(wild.sum()), 1)))
    return np.minimum(rad, 1.0e6).astype(F)


@functools.lru_cache(maxsize=None)
def inputs(w, h, seed=0):
    """The radiance image [H,W,3] of this size, read-only."""
    rng = np.random.default_rng(104729 * w + 31 * h + seed)
    rad = _noisy_ramp(w, h, rng)
    lo, hi = EDGE_LEVELS
    if fits(V_EDGE, w, h):
        y0, y1, x0, x1 = V_EDGE
        rad[y0:y1, x0:x1] = lo
        rad[y0:y1, (x0 + x1) // 2:x1] = hi
    if fits(H_EDGE, w, h):
        y0, y1, x0, x1 = H_EDGE
        rad[y0:y1, x0:x1] = lo
        rad[(y0 + y1) // 2:y1, x0:x1] = hi
    if fits(DIAGONAL, w, h):
        y0, y1, x0, x1 = DIAGONAL
        yy, xx = np.mgrid[y0:y1, x0:x1]
        rad[y0:y1, x0:x1] = np.where(xx - yy > 10, hi, lo)[..., None].astype(F)
    if fits(CHECKER, w, h):
        y0, y1, x0, x1 = CHECKER
        yy, xx = np.mgrid[y0:y1, x0:x1]
        rad[y0:y1, x0:x1] = np.where((xx + yy) & 1, 0.9, 0.1)[..., None].astype(F)
    if fits(SATURATED, w, h):
        y0, y1, x0, x1 = SATURATED
        rad[y0:y1, x0:x1, 1:] = 0.0
    if fits(BLACK, w, h):
        y0, y1, x0, x1 = BLACK
        rad[y0:y1, x0:x1] = 0.0
        rad[LIT] = (0.5, 0.25, 1.5)
    if fits(ISOLUMINANT, w, h):
        y0, y1, x0, x1 = ISOLUMINANT
        yy, xx = np.mgrid[y0:y1, x0:x1]
        rad[y0:y1, x0:x1, :2] = 0.5
        rad[y0:y1, x0:x1, 2] = ((1 + (7 * xx + 3 * yy) % 5) * 1.0e-30).astype(F)
    for y0, y1, x0, x1, axis, at in SEAM_EDGES:
        if fits((y0, y1, x0, x1), w, h):
            rad[y0:y1, x0:x1] = 0.2
            if axis == "x":
                rad[y0:y1, at:x1] = 1.5
            else:
                rad[at:y1, x0:x1] = 1.5
    for (y, x), value in list(UNUSABLE.items()) + list(USABLE_ODDITIES.items()):
        if y < h and x < w:
            rad[y, x] = value
    for y, x in SEAM_UNUSABLE:
        if y < h and x < w:
            rad[y, x] = (0.5, np.nan, 0.5) if (x + y) & 1 else (np.inf, 0.5, 0.5)
    rad.setflags(write=False)
    return rad


def cross(y, x, w, h):
    """The cross neighbours of (y, x) inside the image."""
    return [(qy, qx) for qy, qx in ((y - 1, x), (y, x - 1), (y, x + 1), (y + 1, x)) if 0 <= qy < h and 0 <= qx < w]


def corners(y, x, w, h):
    """The diagonal neighbours of (y, x) inside the image."""
    return [(qy, qx) for qy, qx in ((y - 1, x - 1), (y - 1, x + 1), (y + 1, x - 1), (y + 1, x + 1)) if 0 <= qy < h and 0 <= qx < w]


def reference(rad, p, **kw):
    return R.sharpen(rad, strength=p.strength, flags=p.flags, **kw)


def assert_same(got, want):
    """rgb8 and the radiance's bits."""
    (g8, g), (w8, w) = got[:2], want[:2]
    if g is not None and w is not None:
        assert np.array_equal(R.bits(g), R.bits(w)), f"{(R.bits(g) != R.bits(w)).sum()} radiance values differ"
    if g8 is not None and w8 is not None:
        assert np.array_equal(g8, w8), f"{(g8 != w8).sum()} bytes differ"
