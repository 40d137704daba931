"""What the ff_color_grade tests on the host and on the GPU share: the LUTs, the parameter sets, the seeded images with their planted
special values, and the bitwise comparison.

An image is seeded noise over a little more than the LUT's ranges, with these values planted in its first pixels, as grey pixels
(all three channels equal), as pixels with exactly two equal channels (the tetrahedron's ties) and as mixed ones: every lattice
point's coordinate with its two float neighbours, both domain ends and values outside them, every curve knot's position (LINEAR)
or bit pattern (LOG) with its two float neighbours, the binade boundaries of the LOG axis, negative values, -0 and denormals."""
import functools

import numpy as np

import color_grade_ref as R
from gpupathtracer_amd import lib
from gpupathtracer_amd import types as T

F = np.float32
STAGE_FLAGS = [s for s in range(8)]                                  # every combination of PRIMARY, CURVES, LUT3D ...
FLAG_SETTINGS = STAGE_FLAGS + [s | R.TRILINEAR for s in STAGE_FLAGS if s & R.LUT3D]  # ... and TRILINEAR where it matters
AXES = (R.AXIS_LINEAR, R.AXIS_LOG)
# a white balance with a channel mixer, an offset that makes negatives, a desaturation
PRIMARY_FIELDS = dict(matrix=(1.1, -0.05, 0.02, 0.03, 0.9, -0.01, -0.02, 0.04, 1.25), offset=(-0.02, 0.01, 0.03), saturation=0.7)
# the domain of the lattice per size: the unit cube, one that differs per channel, one with negative ends
DOMAINS = {2: ((0.0, 0.0, 0.0), (1.0, 1.0, 1.0)), 3: ((-0.5, 0.0, 0.125), (1.5, 1.0, 2.0))}
DEFAULT_DOMAIN = ((-0.25, -0.25, -0.25), (1.25, 1.25, 1.25))
LINEAR_RANGE = (-0.25, 1.5)


def from_bits(u):
    return np.array([u], np.uint32).view(F)[0]


def log_axis(K):
    """(lo, hi, shift) of a LOG axis with K knots: 2 and 3 knots a binade apart, else 2^(23 - shift) knots to a binade from 2^-8."""
    if K <= 3:
        shift, lo = 23, F(0.25)
    elif K <= 256:
        shift, lo = 20, F(2.0 ** -8)
    else:
        shift, lo = 16, F(2.0 ** -16)
    hi = from_bits(int(F(lo).view(np.uint32)) + ((K - 1) << shift))
    return float(lo), float(hi), shift


@functools.lru_cache(maxsize=None)
def make_lut(N, K, axis, constant=None):
    """The GradeLut of this key with both halves (N or K 0: without that half): smooth, not affine, not monotone, with negative
    values.  constant: every knot and every texel is this value."""
    rng = np.random.default_rng(1000 * N + K + 7 * axis)
    curves = table = None
    kw = {}
    if K:
        x = np.linspace(0.0, 1.0, K)
        curves = np.stack([x ** 0.8, 0.05 + 0.9 * x * x, 1.1 * x - 0.1]) + rng.uniform(-0.02, 0.02, (3, K))
        if constant is not None:
            curves[:] = constant
        if axis == R.AXIS_LOG:
            lo, hi, shift = log_axis(K)
            kw.update(curve_lo=lo, curve_hi=hi, curve_axis=R.AXIS_LOG, curve_shift=shift)
        else:
            kw.update(curve_lo=LINEAR_RANGE[0], curve_hi=LINEAR_RANGE[1])
    if N:
        g = np.linspace(0.0, 1.0, N)
        b, gg, r = np.meshgrid(g, g, g, indexing="ij")
        table = np.stack([0.9 * r + 0.1 * gg * b, 0.8 * gg + 0.3 * r * r - 0.1, 1.2 * b - 0.2 * r * gg], axis=-1) + rng.uniform(-0.05, 0.05, (N, N, N, 3))
        if constant is not None:
            table[:] = constant
        dmin, dmax = DOMAINS.get(N, DEFAULT_DOMAIN)
        kw.update(domain_min=dmin, domain_max=dmax)
    return lib.grade_lut(curves=curves, table=table, **kw)


def neighbours(v):
    v = np.asarray(v, F)
    return np.concatenate([np.nextafter(v, F(-np.inf)), v, np.nextafter(v, F(np.inf))]).astype(F)


def special_values(lut):
    """The scalars the module's docstring lists, float32 [n]."""
    d = lut.desc
    vals = [np.array([-0.0, 0.0, -1.0e-3, -0.75, -3.0, 1.0e-45, -1.0e-45, 1.0e-39, 1.1754944e-38, 1.0, 7.5, 1.0e6, -1.0e6], F)]
    if d.size:
        for ch in range(3):
            lo, hi = F(d.domain_min[ch]), F(d.domain_max[ch])
            pts = (lo + (hi - lo) * (np.arange(d.size, dtype=np.float64) / (d.size - 1))).astype(F)
            vals += [neighbours(pts), np.array([lo - F(1.0), hi + F(1.0)], F)]
    if d.curve_size:
        lo, hi, K = F(d.curve_lo), F(d.curve_hi), d.curve_size
        step = max(1, K // 16)
        ks = np.unique(np.concatenate([np.arange(0, K, step), [K - 2, K - 1]]))
        if d.curve_axis == R.AXIS_LOG:
            knots = (int(F(lo).view(np.uint32)) + (ks.astype(np.int64) << d.curve_shift)).astype(np.uint32).view(F)
            binades = F(2.0) ** np.arange(np.ceil(np.log2(lo)), np.floor(np.log2(hi)) + 1).astype(F)
            vals += [neighbours(knots), neighbours(binades[::max(1, len(binades) // 8)])]
        else:
            vals += [neighbours((lo + (hi - lo) * (ks / (K - 1))).astype(F))]
        vals += [np.array([lo * F(0.5) - F(0.5), hi * F(2.0) + F(1.0)], F)]
    return np.unique(np.concatenate(vals).view(np.uint32)).view(F)  # (by bit pattern: -0 and +0 both stay)


@functools.lru_cache(maxsize=None)
def inputs(w, h, lut=None, seed=0):
    """The finite image [H,W,3] of this size for this LUT, read-only: the planted pixels first, then noise."""
    rng = np.random.default_rng(7919 * w + 31 * h + seed)
    rad = rng.uniform(-0.4, 1.7, (h * w, 3)).astype(F)
    rad[rng.random(h * w) < 0.05] *= F(40.0)
    sv = special_values(lut) if lut is not None else special_values(make_lut(3, 3, R.AXIS_LINEAR))
    other = np.roll(sv, 5)
    planted = [np.stack([sv, sv, sv], -1), np.stack([sv, sv, other], -1), np.stack([sv, other, sv], -1), np.stack([other, sv, sv], -1),
               np.stack([sv, other, np.roll(sv, 11)], -1)]
    planted = np.concatenate(planted)
    # (a small image takes an even spread of the planted pixels, a large one all of them)
    take = planted if len(planted) <= h * w else planted[np.linspace(0, len(planted) - 1, h * w).astype(int)]
    rad[:len(take)] = take
    rad = rad.reshape(h, w, 3)
    rad.setflags(write=False)
    return rad


def params(flags, lut_id=-1):
    return lib.grade_params(flags=flags, lut_id=lut_id, **PRIMARY_FIELDS)


def flags_id(flags):
    names = [n for bit, n in ((R.PRIMARY, "primary"), (R.CURVES, "curves"), (R.LUT3D, "lut3d"), (R.TRILINEAR, "trilinear")) if flags & bit]
    return "+".join(names) or "copy"


def planted_non_finite(rad, places):
    """A copy of rad with one channel after the other of the given flat pixel indices set to NaN, +Inf, -Inf in turn."""
    out = np.array(rad).reshape(-1, 3)
    for n, i in enumerate(places):
        out[i, n % 3] = (np.nan, np.inf, -np.inf)[n % 3]
    return out.reshape(rad.shape)


def assert_same(got, want):
    """rgb8 and the radiance's bits."""
    (g8, g), (w8, w) = got[:2], want[:2]
    if g is not None and w is not None:
        assert g.shape == w.shape and np.array_equal(R.bits(g), R.bits(w)), f"{(R.bits(g) != R.bits(w)).sum()} radiance values differ"
    if g8 is not None and w8 is not None:
        assert g8.shape == w8.shape and np.array_equal(g8, w8), f"{(g8 != w8).sum()} bytes differ"


# the launch (types.py): the smallest pixel count whose quads one pass of the persistent grid does not cover, and then some
ONE_PASS_PIXELS = T.GRADE_MAX_BLOCKS * T.GRADE_THREADS * T.GRADE_PIXELS_PER_LANE
