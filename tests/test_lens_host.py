"""ff_lens on the host side: exports, defaults, the host twin ff_lens_host - the kernel's per-pixel functions compiled for the host -
bit for bit against the numpy float32 restatement (tests/lens_ref.py) over sizes and parameter sets, the tables against the closed
form in float64, the map against the float64 model, the round trip, the identities the header states, a hand-derived geometric
case, ff_lens_fit_zoom, and every refusal."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from gpupathtracer_amd import lib
from gpupathtracer_amd import types as T
import lens_ref as R
from lens_cases import (BIG, MAP_BOUND_PX, MAP_SETS, MAP_SIZES, PARAMETER_SETS, PLANT_SIZE, ROUND_TRIP_BOUND_PX, ROUND_TRIP_SETS, SIZES, assert_same,
                        geometry_on, inputs, instantiation, params, reference)

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = list(PARAMETER_SETS)


def centres(w, h):
    y, x = np.mgrid[0:h, 0:w]
    return np.stack([x.ravel() + 0.5, y.ravel() + 0.5], axis=1)


def test_new_entry_points_are_exported_and_declared(ff):
    handle = ff.load()
    header = open(os.path.join(ROOT, "include", "firefly", "ff_api.h")).read()
    declared = set(re.findall(r"FF_API\s+[\w\s\*]+?\b(ff_\w+)\s*\(", header))
    for name in ("ff_lens_params_init", "ff_lens", "ff_lens_host", "ff_lens_tables", "ff_lens_map_host", "ff_lens_fit_zoom"):
        assert name in ff.EXPORTS and name in declared and hasattr(handle, name), name
    assert handle.ff_version() == 200


def test_lens_params_defaults_and_size():
    p = lib.lens_params()
    assert (p.k1, p.k2, p.k3, p.center_x, p.center_y, p.zoom, p.ca_red, p.ca_blue, p.vignette, p.vignette_falloff) == (0, 0, 0, 0, 0, 1, 0, 0, 0, 0)
    assert (p.direction, p.filter, p.border, p.flags, p.reserved) == (T.LENS_UNDISTORT, T.LENS_CATMULL_ROM, T.LENS_BORDER_BLACK, T.LENS_ANTI_RING, 0)
    assert C.sizeof(T.FfLensParams) == T.LENS_PARAMS_BYTES == 60
    types_h = open(os.path.join(ROOT, "include", "firefly", "ff_types.h")).read()
    assert "static_assert(sizeof(FfLensParams) == 60" in types_h and "_Static_assert(sizeof(FfLensParams) == 60" in types_h
    assert re.search(r"#define\s+FF_LENS_KNOTS\s+1024\b", types_h) and T.LENS_KNOTS == R.KNOTS == 1024
    with pytest.raises(TypeError):
        lib.lens_params(k4=1.0)
    # the parameter sets reach all six instantiations of the kernel
    assert {instantiation(params(n)) for n in NAMES} == {(f, c) for f in (0, 1, 2) for c in (False, True)}


# ---- 1: twin = restatement ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("w,h", SIZES + [BIG], ids=[f"{w}x{h}" for w, h in SIZES + [BIG]])
def test_twin_matches_the_restatement_bit_for_bit(w, h):
    rad = inputs(w, h)
    for name in NAMES:
        p = params(name)
        got = lib.lens_host(rad, p)
        assert_same(got, reference(rad, p))
        if w * h >= 31 * 7:
            assert (R.bits(got[1]) != R.bits(rad)).any(), name  # (the comparison is not one of copies)
    p = params(NAMES[3])
    both = lib.lens_host(rad, p)
    only8, none = lib.lens_host(rad, p, want_out=False)
    assert none is None and np.array_equal(only8, both[0])
    none, only = lib.lens_host(rad, p, want_rgb8=False)
    assert none is None and np.array_equal(R.bits(only), R.bits(both[1]))


# ---- 2: tables and map against the closed form -------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", NAMES)
def test_tables_are_the_closed_form_correctly_rounded(name):
    for w, h in ((320, 180), (33, 9)):
        p = params(name)
        e, gain, r2_max = lib.lens_tables(w, h, p)
        want_e, want_gain = R.model_tables(p, r2_max)
        assert np.array_equal(R.bits(e), R.bits(want_e.astype(F))), name
        assert np.array_equal(R.bits(gain), R.bits(want_gain.astype(F))), name
        # r2_max: the largest r^2 of a pixel centre
        xy = centres(w, h)
        cx, cy = float(F(0.5) * F(w) + F(p.center_x)), float(F(0.5) * F(h) + F(p.center_y))
        r2 = ((xy[:, 0] - cx) ** 2 + (xy[:, 1] - cy) ** 2) / (0.25 * (w * w + h * h))
        assert r2_max == r2.max()
    assert (lib.lens_tables(64, 36, params(name, vignette=0.0))[1] == F(1.0)).all()
    ident = lib.lens_tables(64, 36)
    assert not ident[0].any() and (ident[1] == F(1.0)).all()


def test_the_map_stays_close_to_the_float64_model():
    worst = {}
    for w, h in MAP_SIZES:
        xy = centres(w, h)
        worst[(w, h)] = 0.0
        for name in MAP_SETS:
            p = params(name)
            tables = lib.lens_tables(w, h, p)
            for channel, want in zip((0, 1, 2), R.model_map(w, h, p, xy, (0, 1, 2))):
                got = lib.lens_map(w, h, xy, p, channel)
                if (w, h) == MAP_SIZES[0]:
                    assert np.array_equal(R.bits(got), R.bits(R.map_positions(w, h, p, tables, xy, channel)))  # the twin's steps 1 and 2
                worst[(w, h)] = max(worst[(w, h)], float(np.abs(got - want).max()))
    print("largest distance of ff_lens_map_host from the float64 model, source pixels:", worst)
    assert max(worst.values()) <= MAP_BOUND_PX
    assert MAP_BOUND_PX < 0.01


def test_undistort_inverts_distort():
    worst = 0.0
    for w, h in MAP_SIZES:
        xy = centres(w, h)
        for fields in ROUND_TRIP_SETS:
            pd, pu = params(fields, direction=T.LENS_DISTORT), params(fields, direction=T.LENS_UNDISTORT)
            model_mid = R.model_map(w, h, pd, xy)
            model_out = ~((model_mid[:, 0] >= 0) & (model_mid[:, 0] <= w) & (model_mid[:, 1] >= 0) & (model_mid[:, 1] <= h))
            assert model_out.mean() <= 0.20, fields  # (the float64 model alone)
            mid = lib.lens_map(w, h, xy, pd)
            keep = (mid[:, 0] >= 0) & (mid[:, 0] <= w) & (mid[:, 1] >= 0) & (mid[:, 1] <= h)
            assert 1.0 - keep.mean() <= 0.20, fields
            back = lib.lens_map(w, h, mid[keep], pu).astype(np.float64)
            worst = max(worst, float(np.abs(back - xy[keep]).max()))
    print("largest round-trip error, pixels:", worst)
    assert worst <= ROUND_TRIP_BOUND_PX


# ---- 4: identities ---------------------------------------------------------------------------------------------------------------------

def test_identities_bit_for_bit():
    w, h = PLANT_SIZE
    clean = np.array(inputs(w, h, planted=False))
    clean[4, 5] = (-0.0, -2.5, 0.0)  # (finite: a negative zero, a negative value)
    assert np.isfinite(clean).all()
    for filt in (T.LENS_BILINEAR, T.LENS_CATMULL_ROM):
        for flags in (0, T.LENS_ANTI_RING):
            for border in (T.LENS_BORDER_BLACK, T.LENS_BORDER_CLAMP):
                p = lib.lens_params(filter=filt, flags=flags, border=border)
                rgb8, out = lib.lens_host(clean, p)
                assert np.array_equal(R.bits(out), R.bits(clean)) and np.array_equal(rgb8, R.to_u8(clean))
                assert_same((rgb8, out), reference(clean, p))
    # a constant image under any geometry, with CLAMP and the anti-ring clamp (and under bilinear)
    flat = np.empty((h, w, 3), F)
    flat[:] = (0.7, 3.0e4, 1.0e-3)
    for name in NAMES:
        for filt, flags in ((T.LENS_CATMULL_ROM, T.LENS_ANTI_RING), (T.LENS_BILINEAR, 0)):
            p = params(name, filter=filt, flags=flags, border=T.LENS_BORDER_CLAMP, vignette=0.0)
            assert np.array_equal(R.bits(lib.lens_host(flat, p)[1]), R.bits(flat)), name
    rad = inputs(w, h)
    for name in NAMES:
        p = params(name)
        out = lib.lens_host(rad, p)[1]
        # the green channel does not depend on the chromatic aberration
        no_ca = lib.lens_host(rad, params(name, ca_red=0.0, ca_blue=0.0))[1]
        with_ca = lib.lens_host(rad, params(name, ca_red=0.01, ca_blue=-0.02))[1]
        assert np.array_equal(R.bits(no_ca[..., 1]), R.bits(with_ca[..., 1])) and np.array_equal(R.bits(out[..., 1]), R.bits(no_ca[..., 1]))
        assert not np.array_equal(R.bits(no_ca[..., 0]), R.bits(with_ca[..., 0]))
        # vignette 0 leaves the geometry's result; with it, the result is that times the gain
        plain = lib.lens_host(rad, params(name, vignette=0.0))[1]
        d = reference(rad, p, details=True)[2]
        assert np.array_equal(R.bits(out), R.bits(plain * d["gain"][..., None]))


def test_vignette_alone_is_the_input_times_the_gain():
    """Geometry off: out = in * g.  By hand, 65 x 17, DISTORT, vignette 0.8, falloff 0.9: at the centre pixel (32, 8) r = 0 and
    g = (1 - 0.8) + 0.8 * 1 = 1; at the corner pixel (0, 0) r^2 = r2_max = (32^2 + 8^2) / (32.5^2 + 8.5^2) = 1088 / 1128.5,
    (F r)^2 = 0.81 * 0.964112 = 0.780930, v = 1 / 1.780930^2 = 0.315286 and g = 0.2 + 0.8 * 0.315286 = 0.452229."""
    w, h = PLANT_SIZE
    rad = inputs(w, h, planted=False)
    p = params("vignette_distort_only")
    out = lib.lens_host(rad, p)[1]
    e, gain, r2_max = lib.lens_tables(w, h, p)
    assert not e.any()
    d = reference(rad, p, details=True)[2]
    assert np.array_equal(R.bits(out), R.bits(rad * d["gain"][..., None]))
    assert r2_max == pytest.approx(1088.0 / 1128.5, rel=1e-12)
    assert d["gain"][8, 32] == F(1.0) and np.array_equal(R.bits(out[8, 32]), R.bits(rad[8, 32]))
    assert d["gain"][0, 0] == gain[-1] and float(gain[-1]) == pytest.approx(0.452229, abs=2e-6)
    assert np.array_equal(R.bits(out[0, 0]), R.bits(rad[0, 0] * gain[-1]))
    # UNDISTORT removes what DISTORT added: the reciprocal
    back = lib.lens_tables(w, h, params("vignette_distort_only", direction=T.LENS_UNDISTORT))[1]
    assert np.allclose(back.astype(np.float64) * gain.astype(np.float64), 1.0, rtol=2e-7, atol=0.0)


# ---- 5: a hand-derived geometric case ---------------------------------------------------------------------------------------------------

def test_a_bright_pixel_lands_where_the_paper_says():
    """33 x 1, k1 = 0.2376, UNDISTORT, bilinear: c = (16.5, 0.5), D2 = 0.25 (33^2 + 1) = 272.5.  The only bright source pixel is 13,
    centre 13.5.  Output pixel x has dx = x - 16, r^2 = dx^2 / 272.5 and its source is px + dx k1 r^2 = px + k1 dx^3 / 272.5 (e is
    linear in r^2, so the table interpolates it exactly).  x = 6: dx = -10, shift = -0.2376 * 1000 / 272.5 = -0.87193: source 5.628.
    Wanted: the x whose taps include pixel 13.  x = 13: dx = -3, shift = 0.2376 * -27 / 272.5 = -0.023542, source 13.476458,
    u = source - 0.5 = 12.976458: taps 12 and 13 with fraction 0.976458, so pixel 13 weighs 0.976458.  x = 14: dx = -2, shift =
    -0.006975, u = 13.993025: taps 13 and 14 with fraction 0.993025, so pixel 13 weighs 0.006975.  x = 12: dx = -4, shift =
    -0.055804, u = 11.944196: taps 11 and 12, nothing.  So the output is 100 * 0.976458 at column 13, 100 * 0.006975 at column 14
    and 0 elsewhere: undistorting a pincushion pulls the picture outward, by 0.0235 px at this radius."""
    w = 33
    rad = np.zeros((1, w, 3), F)
    rad[0, 13] = 100.0
    out = lib.lens_host(rad, lib.lens_params(k1=0.2376, direction=T.LENS_UNDISTORT, filter=T.LENS_BILINEAR, flags=0, border=T.LENS_BORDER_CLAMP))[1]
    lit = np.nonzero(out[0, :, 1])[0]
    assert list(lit) == [13, 14]
    assert float(out[0, 13, 1]) == pytest.approx(100.0 * (1.0 - 0.2376 * 27.0 / 272.5), rel=2e-6)
    assert float(out[0, 14, 1]) == pytest.approx(100.0 * (0.2376 * 8.0 / 272.5), rel=2e-4)
    src = lib.lens_map(w, 1, [[6.5, 0.5]], lib.lens_params(k1=0.2376))
    assert float(src[0, 0]) == pytest.approx(6.5 - 0.2376 * 1000.0 / 272.5, abs=2e-6) and src[0, 1] == F(0.5)


# ---- 6: ff_lens_fit_zoom ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", NAMES[:6])
def test_fit_zoom(name):
    w, h = 64, 36
    ones = np.ones((h, w, 3), F)
    fields = dict(PARAMETER_SETS[name], border=T.LENS_BORDER_BLACK, vignette=0.0, ca_red=0.0, ca_blue=0.0)
    fill = lib.lens_fit_zoom(w, h, params(fields), T.LENS_FIT_FILL)
    assert lib.lens_fit_zoom(w, h, params(fields, zoom=3.0), T.LENS_FIT_FILL) == fill  # (p->zoom is not read)
    out = lib.lens_host(ones, params(fields, zoom=fill))[1]
    assert (out[..., 1] > F(0.5)).all(), "a border shows at the FILL zoom"  # (1 up to the weights' rounding, or the border's 0)
    out = lib.lens_host(ones, params(fields, zoom=fill * 0.99))[1]
    assert (out[..., 1] == F(0.0)).any(), "no border shows 1 % below the FILL zoom"
    # ALL: the four corners of the source map inside the output - found through the opposite direction's map of the same lens
    zall = lib.lens_fit_zoom(w, h, params(fields), T.LENS_FIT_ALL)
    assert zall <= fill
    p = params(fields, zoom=zall)
    k = (p.k1, p.k2, p.k3)
    cx, cy, d = w / 2 + p.center_x, h / 2 + p.center_y, np.sqrt(0.25 * (w * w + h * h))
    for sx, sy in ((0.0, 0.0), (w, 0.0), (0.0, h), (w, h)):
        r = np.hypot(sx - cx, sy - cy) / d
        rho = R.model_f_inverse(k, r) if p.direction == T.LENS_UNDISTORT else R.model_f(k, r)
        ox, oy = cx + (sx - cx) * zall * rho / r, cy + (sy - cy) * zall * rho / r
        assert 0.0 <= ox <= w and 0.0 <= oy <= h, (name, (sx, sy), (ox, oy))
    with pytest.raises(lib.FireflyError) as e:
        lib.lens_fit_zoom(w, h, params(fields), 2)
    assert "mode" in e.value.message


# ---- 7: refusals -----------------------------------------------------------------------------------------------------------------------

def raw_host(p, rad, rgb8=None, out=None, w=None, h=None):
    ptr = lambda a: a.ctypes.data if a is not None else None  # noqa: E731
    hh, ww = rad.shape[:2] if rad is not None else (15, 17)
    return lib.load().ff_lens_host(ww if w is None else w, hh if h is None else h, C.byref(p) if p is not None else None, ptr(rad), ptr(rgb8), ptr(out))


def test_every_refused_argument_names_its_field():
    rad = np.array(inputs(17, 15))
    out = np.full(rad.shape, 7.0, F)
    last = lambda: lib.load().ff_last_error().decode()  # noqa: E731
    nan, inf = float("nan"), float("inf")
    cases = []
    for field, bad in [("k1", (10.5, -11.0)), ("k2", (10.5,)), ("k3", (-10.5,)), ("center_x", (8.6, -9.0)), ("center_y", (7.6, -7.6)),
                       ("zoom", (0.0, 0.06, 16.5, -1.0)), ("ca_red", (0.3, -0.3)), ("ca_blue", (0.26,)), ("vignette", (-0.1, 1.1)),
                       ("vignette_falloff", (-0.5, 8.5))]:
        cases += [(field, v) for v in bad + (nan, inf, -inf)]
    cases += [("direction", 2), ("direction", -1), ("filter", 2), ("border", 2), ("border", -1), ("reserved", 1), ("flags", 2), ("flags", 0x80000001)]
    for field, value in cases:
        assert raw_host(lib.lens_params(**{field: value}), rad, None, out) == T.FF_ERR_INVALID_ARG, (field, value)
        assert field in last(), (field, value, last())
    # reserved is named before the flags
    assert raw_host(lib.lens_params(reserved=1, flags=2), rad, None, out) == T.FF_ERR_INVALID_ARG and "reserved" in last()
    for field, value in [("k1", 10.0), ("center_x", 8.5), ("zoom", 16.0), ("zoom", 0.0625), ("vignette", 1.0), ("ca_red", -0.25)]:  # (the ends are allowed)
        assert raw_host(lib.lens_params(**{field: value, "direction": T.LENS_UNDISTORT if field != "k1" else T.LENS_DISTORT}), rad, None, out) == T.FF_OK, (
            field, last())
    out[:] = 7.0
    # a fold-over: the message names the radius.  f(s) = s (1 - 0.5 s^2) stops rising at s = sqrt(2 / 3) = 0.8165, where f = 0.5443
    for direction in (T.LENS_UNDISTORT, T.LENS_DISTORT):
        assert raw_host(lib.lens_params(k1=-0.5, direction=direction), rad, None, out) == T.FF_ERR_INVALID_ARG
        assert "fold" in last() and "radius 0.81649" in last(), last()
    assert raw_host(lib.lens_params(k1=-0.5, zoom=1.25, direction=T.LENS_UNDISTORT), rad, None, out) == T.FF_OK  # (the range ends at 0.776)
    assert raw_host(lib.lens_params(k1=-0.5, zoom=2.0, direction=T.LENS_DISTORT), rad, None, out) == T.FF_OK     # (f reaches 0.485 before the fold)
    assert raw_host(lib.lens_params(k1=0.3, k2=-0.6), rad, None, out) == T.FF_ERR_INVALID_ARG and "radius" in last()
    for entry in (lambda q: lib.lens_tables(17, 15, q), lambda q: lib.lens_map(17, 15, [[1.0, 1.0]], q), lambda q: lib.lens_fit_zoom(17, 15, q, 2)):
        with pytest.raises(lib.FireflyError):
            entry(lib.lens_params(k1=11.0))
    with pytest.raises(lib.FireflyError) as e:
        lib.lens_tables(17, 15, lib.lens_params(k1=-0.5))
    assert "radius" in e.value.message
    with pytest.raises(lib.FireflyError) as e:
        lib.lens_map(17, 15, [[nan, 1.0]])
    assert "xy_out" in e.value.message
    with pytest.raises(lib.FireflyError) as e:
        lib.lens_map(17, 15, [[1.0, 1.0]], channel=3)
    assert "channel" in e.value.message
    out[:] = 7.0
    p = lib.lens_params(k1=-0.1)
    for args, word in [((None, rad), "params"), ((p, None), "radiance_in")]:
        assert raw_host(*args, None, out, w=17, h=15) == T.FF_ERR_INVALID_ARG and word in last(), (word, last())
    for w, h in [(0, 15), (17, 0), (65536, 1), (1, 65536), (-1, 3)]:
        assert raw_host(p, rad, None, out, w=w, h=h) == T.FF_ERR_INVALID_ARG and "size" in last()
    # overlapping buffers: this is a gather
    assert raw_host(p, rad, None, rad) == T.FF_ERR_INVALID_ARG and "radiance_out overlaps radiance_in" in last()
    assert raw_host(p, rad, None, rad.reshape(-1)[3:]) == T.FF_ERR_INVALID_ARG and "radiance_out overlaps radiance_in" in last()
    assert raw_host(p, rad, rad.view(np.uint8), out) == T.FF_ERR_INVALID_ARG and "rgb8 overlaps radiance_in" in last()
    assert raw_host(p, rad, out.view(np.uint8), out) == T.FF_ERR_INVALID_ARG and "rgb8 overlaps radiance_out" in last()
    assert (out == 7.0).all() and np.array_equal(R.bits(rad), R.bits(inputs(17, 15)))
    # the device entry point refuses a NULL state, and the same arguments, before it touches a device
    d = lib.load().ff_lens
    assert d(None, 17, 15, C.byref(p), rad.ctypes.data, 0, None, 0, out.ctypes.data, 0) == T.FF_ERR_INVALID_ARG
    assert "state" in last()
    assert geometry_on(p)
