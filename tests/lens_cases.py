"""What the ff_lens tests on the host and on the GPU share: the image sizes, the parameter sets, the seeded images with their planted
pixels and the bitwise comparison.

Every image is deterministic noise about a ramp with HDR outliers up to 1e4.  The kernel works on tiles of 32 x 8 output pixels:
PLANTED puts NaN, +Inf, -Inf and negative pixels on both sides of the seams x = 31 | 32 and y = 7 | 8 into every image large enough
to hold them."""
import functools

import numpy as np

from gpupathtracer_amd import lib
from gpupathtracer_amd import types as T
import lens_ref as R

F = np.float32
# (w, h): the 1-pixel image, one smaller than a tile in both axes, image edges inside, on and just past a tile edge, more than one
# tile in both axes, a 16:9 frame of two tiles by five
SIZES = [(1, 1), (2, 3), (31, 7), (32, 8), (33, 9), (65, 17), (64, 36)]
BIG = (320, 180)
PLANT_SIZE = (65, 17)

U, D = T.LENS_UNDISTORT, T.LENS_DISTORT
BL, CR = T.LENS_BILINEAR, T.LENS_CATMULL_ROM
BLACK, CLAMP = T.LENS_BORDER_BLACK, T.LENS_BORDER_CLAMP
RING = T.LENS_ANTI_RING

# name -> the fields that differ from the identity.  Together: barrel (k1 < 0) and pincushion (k1 > 0) in both directions, k2 and k3,
# an off-centre c, zoom != 1, CA on one channel and on both with opposite signs, the vignette in both directions, both borders, the
# three filter forms (bilinear, Catmull-Rom, Catmull-Rom with the clamp) with shared and with per-channel positions: all six
# instantiations of the kernel.
PARAMETER_SETS = {
    "barrel_undistort_cr_ring": dict(k1=-0.12, direction=U, filter=CR, flags=RING, border=BLACK),
    "barrel_distort_bilinear": dict(k1=-0.12, direction=D, filter=BL, flags=0, border=CLAMP),
    "pincushion_undistort_cr": dict(k1=0.15, direction=U, filter=CR, flags=0, border=CLAMP),
    "pincushion_distort_cr_ring_ca": dict(k1=0.15, direction=D, filter=CR, flags=RING, border=BLACK, ca_red=0.004, ca_blue=-0.003),
    "k2_k3_offcentre_zoom_bilinear_ca": dict(k1=-0.08, k2=0.03, k3=-0.01, center_x=0.4, center_y=-0.3, zoom=1.08, direction=D, filter=BL, flags=0,
                                             border=BLACK, ca_red=-0.006),
    "k2_k3_undistort_cr_ca_vignette": dict(k1=0.05, k2=-0.02, k3=0.004, zoom=0.93, direction=U, filter=CR, flags=0, border=CLAMP, ca_blue=0.005,
                                           vignette=0.6, vignette_falloff=1.1),
    "vignette_distort_only": dict(direction=D, filter=CR, flags=RING, vignette=0.8, vignette_falloff=0.9),
    "vignette_undistort_zoom": dict(zoom=1.25, direction=U, filter=BL, flags=0, vignette=0.5, vignette_falloff=1.3, border=BLACK),
}


def params(name_or_fields, **more):
    fields = dict(PARAMETER_SETS[name_or_fields]) if isinstance(name_or_fields, str) else dict(name_or_fields)
    fields.update(more)
    return lib.lens_params(**fields)


def instantiation(p):
    """(filter form, per-channel positions) - the kernel's template arguments for p."""
    form = 0 if p.filter == BL else (2 if p.flags & RING else 1)
    return form, bool(p.ca_red != 0.0 or p.ca_blue != 0.0)


def geometry_on(p):
    return any(v != 0.0 for v in (p.k1, p.k2, p.k3, p.ca_red, p.ca_blue)) or p.zoom != 1.0


# (y, x) -> the pixel planted there: beside x = 31 | 32 and y = 7 | 8, on both sides of each
PLANTED = {(3, 31): (np.nan, 0.5, 0.25), (5, 32): (np.inf, 1.0, 1.0), (7, 12): (0.5, -np.inf, 0.5), (8, 20): (-0.75, -0.5, -0.25),
           (7, 31): (1.0, np.nan, -np.inf), (8, 32): (-1.5, np.inf, np.nan), (12, 31): (-2.0, 0.25, 0.5), (2, 32): (0.5, 0.5, np.nan)}


def _noise(w, h, rng):
    y, x = np.mgrid[0:h, 0:w]
    base = 0.1 + 0.9 * x / max(w, 1) + 0.5 * y / max(h, 1)
    rad = base[..., None] * np.array([1.0, 0.8, 0.6]) * rng.uniform(0.5, 1.5, (h, w, 3))
    wild = rng.random((h, w)) < 0.04
    rad[wild] *= np.power(10.0, rng.uniform(1.0, 4.0, (int(wild.sum()), 1)))
    return rad.astype(F)


@functools.lru_cache(maxsize=None)
def inputs(w, h, seed=0, planted=True):
    """The radiance image [H,W,3] of this size, read-only; planted=False: the same image without the PLANTED pixels (finite, > 0)."""
    rng = np.random.default_rng(7919 * w + 131 * h + seed)
    rad = _noise(w, h, rng)
    if planted:
        for (y, x), value in PLANTED.items():
            if y < h and x < w:
                rad[y, x] = value
    rad.setflags(write=False)
    return rad


def reference(rad, p, **kw):
    h, w = rad.shape[:2]
    return R.lens(rad, p, lib.lens_tables(w, h, p), **kw)


def assert_same(got, want):
    """rgb8 and the radiance's bits."""
    (g8, g), (w8, w) = got[:2], want[:2]
    if g is not None and w is not None:
        assert np.array_equal(R.bits(g), R.bits(w)), f"{(R.bits(g) != R.bits(w)).sum()} radiance values differ"
    if g8 is not None and w8 is not None:
        assert np.array_equal(g8, w8), f"{(g8 != w8).sum()} bytes differ"


# ---- the map's accuracy ---------------------------------------------------------------------------------------------------------------
# Parameter sets for the accuracy of ff_lens_map_host against the float64 model, and for the round trip.  MAP_BOUND_PX and
# ROUND_TRIP_BOUND_PX are TWICE the maxima measured on the CPU with the twin over these sets at 320 x 180 and 1920 x 1080 (the
# margin covers other parameter sets); the measured values stand in DESIGN.md section 8 row 26 and are printed by the tests.
MAP_SETS = ["barrel_undistort_cr_ring", "barrel_distort_bilinear", "pincushion_undistort_cr", "pincushion_distort_cr_ring_ca",
            "k2_k3_offcentre_zoom_bilinear_ca", "k2_k3_undistort_cr_ca_vignette"]
MAP_SIZES = [(320, 180), (1920, 1080)]
MAP_MEASURED_PX = 2.8e-4         # 2.76e-4 px: barrel_distort_bilinear at 1920 x 1080 (3.5e-5 px at 320 x 180)
ROUND_TRIP_MEASURED_PX = 1.3e-4  # 1.22e-4 px at 1920 x 1080: one float32 ulp of a coordinate above 1024
MAP_BOUND_PX, ROUND_TRIP_BOUND_PX = 2.0 * MAP_MEASURED_PX, 2.0 * ROUND_TRIP_MEASURED_PX
# coefficients of the round trip map(UNDISTORT) o map(DISTORT): with these the float64 model alone sends under 20 % of the pixel
# centres outside the image on the way (checked in test_lens_host.py)
ROUND_TRIP_SETS = [dict(k1=-0.12), dict(k1=0.15), dict(k1=-0.08, k2=0.03, k3=-0.01, center_x=0.4, center_y=-0.3), dict(k1=0.05, k2=-0.02, k3=0.004)]
