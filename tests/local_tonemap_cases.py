"""The inputs the ff_local_tonemap tests share (tests/test_local_tonemap_host.py, tests/test_gpu_local_tonemap.py): seeded random HDR
images, the spoiled pixels, the two-region image and its checker variant, images in the first and the last stop whose cell sums
pass 2^24, a checker of two bins, a pair of images of which the second empties chosen cells, and the comparison helpers.  Every
image is built once per size and handed out read-only."""
import functools

import numpy as np

from gpupathtracer_amd import lib
import local_tonemap_ref as R

F = np.float32
CELLS = (8, 16, 32, 64)
COMPRESSIONS = (0.0, 0.5, 1.0)
DETAILS = (0.0, 1.0, 2.0)
HOST_SIZES = [(1, 1), (7, 5), (33, 17), (65, 33), (130, 70), (200, 136)]
# the GPU table: (w, h, cells); None = the default cell.  130 x 70 gives every cell size several cell columns, several cell rows and
# partial last cells at once (17 x 9, 9 x 5, 5 x 3 and 3 x 2 cells); 200 x 136 gives cell 64 a 4 x 3 grid with full tiles inside
GPU_SHAPES = [(1, 1, (None,)), (7, 5, (8,)), (33, 17, (8, 16, 32)), (65, 33, (64,)), (130, 70, (8, 16, 32, 64)), (200, 136, (64,))]
TOL = 2.0 ** -12  # the hand-derived cases' relative tolerance
# cells (cy, cx) of the 130 x 70 image that stale_pair() empties.  Cell 8 packs four tiles to a workgroup (17 columns: four whole
# workgroups and a last one of one tile, 2 pixels wide): one tile of four (the second, the fourth), the last workgroup's only tile,
# and the same in the last, partial cell row
STALE_SIZE = (130, 70)
STALE_CELLS = {8: ((2, 5), (6, 11), (4, 16), (8, 3), (8, 16)), 16: ((1, 2), (4, 8)), 32: ((1, 1), (2, 4)), 64: ((0, 1), (1, 2))}

# what makes a pixel unmapped: non-finite, negative, below 2^-16 (black and -0 among them)
SPOILED = [(np.nan, 1.0, 1.0), (1.0, np.inf, 1.0), (1.0, 1.0, -np.inf), (-0.5, 2.0, 2.0), (3.0, -1e-30, 3.0), (0.0, 0.0, 0.0), (-0.0, -0.0, -0.0),
           (1e-6, 1e-6, 1e-6), (2.0 ** -17, 2.0 ** -17, 2.0 ** -17)]


def bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


def assert_same(got, want):
    """(rgb8, radiance) pairs agree: the bytes, and the floats bit for bit (NaN payloads and the sign of zero included)."""
    assert np.array_equal(got[0], want[0]), f"rgb8 differs at {np.argwhere(got[0] != want[0])[:4].tolist()}"
    diff = bits(got[1]) != bits(want[1])
    assert not diff.any(), f"radiance differs at {np.argwhere(diff)[:4].tolist()}: {got[1][diff][:4]} != {want[1][diff][:4]}"


@functools.lru_cache(maxsize=None)
def hdr(w, h, lo=-12.0, hi=12.0):
    """A seeded random HDR image spanning 2^lo .. 2^hi: smooth large-scale exposure regions with an edge, fine texture on top and
    a tint per pixel, so that the grid has populated and empty cells, neighbouring bins and pixels on bin boundaries."""
    rng = np.random.default_rng(1000 * w + h)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    region = np.where(x + 0.5 * y > 0.55 * (w + 0.5 * h), hi - 3.0, lo + 3.0) + 2.5 * np.sin(x / 9.0) * np.cos(y / 7.0)
    stops = np.clip(region + rng.uniform(-0.5, 0.5, (h, w)), lo, hi)
    pick = rng.random((h, w))
    stops = np.where(pick < 0.05, rng.uniform(lo, hi, (h, w)), stops)              # lone outliers anywhere in the range
    stops = np.where((pick >= 0.05) & (pick < 0.10), np.round(stops), stops)       # exact powers of two: bin boundaries
    tint = rng.uniform(0.25, 1.0, (h, w, 3))
    img = (np.exp2(stops)[..., None] * tint).astype(F)
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def spoiled(w, h):
    """hdr(w, h) with every kind of SPOILED pixel planted (as many as fit), and the list of their places."""
    img = np.array(hdr(w, h))
    rng = np.random.default_rng(77 * w + h)
    places = []
    for k, px in enumerate(SPOILED * 3):
        y, x = int(rng.integers(h)), int(rng.integers(w))
        if (y, x) in places:
            continue
        img[y, x] = px
        places.append((y, x))
    img.setflags(write=False)
    return img, tuple(places)


@functools.lru_cache(maxsize=None)
def two_regions(checker=False):
    """128 x 64 grey: the left half l = 0.125, the right half l = 32 (or a 1-pixel checker of 32 and 40)."""
    img = np.empty((64, 128, 3), F)
    img[:, :64] = 0.125
    img[:, 64:] = 32.0
    if checker:
        y, x = np.mgrid[0:64, 64:128]
        img[:, 64:][(x + y) % 2 == 1] = 40.0
    img.setflags(write=False)
    return img


TWO_REGION_PARAMS = dict(pivot=1.0, compression=0.5, detail=1.0, cell=16)

# the stops at the two ends of the 40-stop range: l in [2^23, 2^24) and in [2^-16, 2^-15)
EXTREME_STOPS = {"top": 2.0 ** 23, "bottom": 2.0 ** -16}


@functools.lru_cache(maxsize=None)
def extreme(stop, two_level):
    """128 x 128 grey (2 x 2 full cells of 64) inside one stop at an end of the range, so that a cell's sum of q10 is about 4096 x
    24 063 or 4096 x -15 873, beyond +-2^24 where (float)int rounds.  The mantissas sit in the middle of a q10 step with an odd q10
    (1 + 511.5 / 1024; the second level 1 + 256.5 / 1024), so that the rounding of the luminance sum cannot move q10.  Flat: one bin,
    one q10, a thread's run as long as the splat allows.  Two levels: the second on every pixel with (5 x + 3 y) % 7 == 0, an
    odd-ish count per cell, so that S is no multiple of the float's step there (the tests assert that it really rounds)."""
    base = EXTREME_STOPS[stop]
    img = np.full((128, 128, 3), base * (1.0 + 511.5 / 1024.0), F)
    if two_level:
        y, x = np.mgrid[0:128, 0:128]
        img[(5 * x + 3 * y) % 7 == 0] = base * (1.0 + 256.5 / 1024.0)
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def bin_checker(rows=0):
    """128 x 128 grey, a one-pixel checker of l = 1.5 and l = 3 (bins 16 and 17): level (x + y) % 2.  rows > 0 shifts the checker by
    one column every `rows` rows: the splat's threads of cell 32 and 64 own a column of pixels 8 and 4 rows apart (256 threads over
    rows of 32 and 64 pixels), and the plain checker has one level down such a column - with rows = 8 or 4 a thread's consecutive
    pixels alternate and no run is longer than one (longest_run() says so)."""
    y, x = np.mgrid[0:128, 0:128]
    level = (x + y + (y // rows if rows else 0)) % 2
    img = np.repeat(np.where(level == 1, F(3.0), F(1.5))[..., None], 3, axis=2).astype(F)
    img.setflags(write=False)
    return img


def longest_run(rad, cell):
    """The longest run of one bin among the consecutive pixels of a thread of the splat: a workgroup of 256 threads strides over its
    cell row by row, so a thread's pixels are one column, 256 / cell rows apart (cells 8 and 16: one pixel per thread)."""
    if cell * cell <= 256:
        return 1
    q10 = R.q16_of(R.luminance(np.asarray(rad, dtype=F))) >> 6
    bins = (q10 >> 10) + 16
    step, (h, w) = 256 // cell, bins.shape
    longest = 1
    for y0 in range(0, h, cell):
        for first in range(step):
            col = bins[y0 + first:min(y0 + cell, h):step]      # [k, w]: the k-th pixel of the threads that start in row `first`
            run = np.ones(col.shape[1], np.int64)
            for k in range(1, col.shape[0]):
                run = np.where(col[k] == col[k - 1], run + 1, 1)
                longest = max(longest, int(run.max()))
    return longest


@functools.lru_cache(maxsize=None)
def stale_pair(cell):
    """(first, second, cells): hdr(130, 70), every pixel mapped, and the same image with the pixels of STALE_CELLS[cell] unmapped."""
    w, h = STALE_SIZE
    first = hdr(w, h)
    second = np.array(first)
    for cy, cx in STALE_CELLS[cell]:
        second[cy * cell:(cy + 1) * cell, cx * cell:(cx + 1) * cell] = (-1.0, 2.0, 3.0)
    second.setflags(write=False)
    return first, second, STALE_CELLS[cell]


def stale_bases(cell):
    """For each emptied cell of stale_pair(cell) the pixel left of its top-left corner, a mapped one: (cell, step 4's base of that
    pixel in the second image, the base it would get if the cell still held the first image's count and sum)."""
    first, second, cells = stale_pair(cell)
    p = params(cell=cell)
    n1, S1 = lib.local_tonemap_grid_host(first, p)
    n2, S2 = lib.local_tonemap_grid_host(second, p)
    ns, Ss = n2.copy(), S2.copy()
    for cy, cx in cells:
        ns[cy, cx], Ss[cy, cx] = n1[cy, cx], S1[cy, cx]
    xs = np.array([cx * cell - 1 for _, cx in cells])
    ys = np.array([cy * cell for cy, _ in cells])
    lf = R.lf_of(R.q16_of(R.luminance(second[ys, xs])))
    true = R.slice_grid(*R.blur(n2, S2), xs, ys, lf, cell)
    stale = R.slice_grid(*R.blur(ns, Ss), xs, ys, lf, cell)
    return list(zip(cells, true.tolist(), stale.tolist()))


@functools.lru_cache(maxsize=None)
def midrange(w, h):
    """An image that stays inside 2^-10 .. 2^16 after scaling by 2^-3 and 2^4: 2^-7 .. 2^11 (the tint takes up to two stops)."""
    return hdr(w, h, -5.0, 11.0)


def params(**kw):
    return lib.local_tonemap_params(**kw)


def fields(p):
    return dict(compression=p.compression, detail=p.detail, pivot=p.pivot, cell=p.cell)


@functools.lru_cache(maxsize=None)
def _reference(key, w, h, compression, detail, pivot, cell):
    img = {"hdr": hdr, "midrange": midrange}[key](w, h)
    res = R.local_tonemap(img, compression, detail, pivot, cell)
    for a in res:
        a.setflags(write=False)
    return res


def reference(rad, p, key=None):
    """The restatement's (rgb8, radiance) for rad under p; cached when rad is hdr(w, h) or midrange(w, h) (key says which)."""
    f = fields(p)
    if key:
        h, w = rad.shape[:2]
        return _reference(key, w, h, f["compression"], f["detail"], f["pivot"], f["cell"])
    return R.local_tonemap(rad, **f)
