"""The inputs the ff_local_tonemap tests share (tests/test_local_tonemap_host.py, tests/test_gpu_local_tonemap.py): seeded random HDR
images, the spoiled pixels, the two-region image and its checker variant, and the comparison helpers.  Every image is built once
per size and handed out read-only."""
import functools

import numpy as np

from gpupathtracer_amd import lib
import local_tonemap_ref as R

F = np.float32
CELLS = (8, 16, 32, 64)
COMPRESSIONS = (0.0, 0.5, 1.0)
DETAILS = (0.0, 1.0, 2.0)
HOST_SIZES = [(1, 1), (7, 5), (33, 17), (65, 33)]
# the GPU table of the issue: (w, h, cells); None = the default cell
GPU_SHAPES = [(1, 1, (None,)), (7, 5, (8,)), (33, 17, (8, 16, 32)), (65, 33, (64,)), (130, 70, (8,))]
TOL = 2.0 ** -12  # the hand-derived cases' relative tolerance

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
