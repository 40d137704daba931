"""ff_despeckle on the host side: exports, defaults, every argument check (all before any device work), the host twin
ff_despeckle_host - the kernel's per-pixel functions compiled for the host - bit for bit against the numpy float32 reference
(tests/despeckle_ref.py) over sizes, radii, ranks, flags and min_neighbours, the consequences the header states, the planted spikes
and the pixels that are never touched."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from gpupathtracer_amd import lib
from gpupathtracer_amd import types as T
import despeckle_ref as R
from despeckle_cases import (BLOCK, PAIRS, PLANT_SIZE, RADII, RANKS, SEAMS, SINGLES, SIZES, assert_same, inputs, planted, ramp, reference)

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAG = T.DESPECKLE_DEMODULATE_ALBEDO


def twin_matches_reference(rad, albedo, ids, p):
    got = lib.despeckle_host(rad, (albedo, ids), p)
    assert_same(got, reference(rad, albedo, ids, p))
    return got


def window(p):
    return (2 * p.radius + 1) ** 2 - 1


def test_new_entry_points_are_exported_and_declared(ff):
    handle = ff.load()
    header = open(os.path.join(ROOT, "include", "firefly", "ff_api.h")).read()
    declared = set(re.findall(r"FF_API\s+[\w\s\*]+?\b(ff_\w+)\s*\(", header))
    for name in ("ff_despeckle_params_init", "ff_despeckle", "ff_despeckle_host"):
        assert name in ff.EXPORTS and name in declared and hasattr(handle, name), name


def test_despeckle_params_defaults_and_size():
    p = lib.despeckle_params()
    assert (p.radius, p.rank, p.min_neighbours, p.threshold, p.floor, p.flags, p.reserved) == (1, 2, 3, 2.0, 0.0, FLAG, 0)
    assert C.sizeof(T.FfDespeckleParams) == T.DESPECKLE_PARAMS_BYTES == 28
    types_h = open(os.path.join(ROOT, "include", "firefly", "ff_types.h")).read()
    assert "static_assert(sizeof(FfDespeckleParams) == 28" in types_h and "_Static_assert(sizeof(FfDespeckleParams) == 28" in types_h
    assert re.search(r"#define\s+FF_DESPECKLE_DEMODULATE_ALBEDO\s+1\b", types_h)
    q = lib.despeckle_params(radius=3, threshold=4.0)
    assert q.radius == 3 and q.threshold == 4.0
    with pytest.raises(TypeError):
        lib.despeckle_params(max_radius=3)


def raw_host(p, rad, albedo, ids, rgb8=None, out=None, w=None, h=None):
    ptr = lambda a: a.ctypes.data if a is not None else None  # noqa: E731
    hh, ww = rad.shape[:2] if rad is not None else (9, 17)
    return lib.load().ff_despeckle_host(ww if w is None else w, hh if h is None else h, C.byref(p) if p is not None else None, ptr(rad), ptr(albedo), ptr(ids),
                                        ptr(rgb8), ptr(out), None)


def test_every_refused_argument_names_its_field():
    rad, albedo, ids = (np.array(a) for a in inputs(17, 15))
    out = np.full(rad.shape, 7.0, F)
    last = lambda: lib.load().ff_last_error().decode()  # noqa: E731
    nan, inf = float("nan"), float("inf")
    cases = [("radius", 0), ("radius", 4), ("rank", 0), ("rank", 5), ("min_neighbours", 1), ("min_neighbours", 9), ("threshold", 0.5), ("threshold", nan),
             ("threshold", inf), ("floor", -1.0), ("floor", nan), ("floor", inf), ("flags", 2), ("flags", 3), ("reserved", 1)]
    for field, value in cases:
        assert raw_host(lib.despeckle_params(**{field: value}), rad, albedo, ids, None, out) == T.FF_ERR_INVALID_ARG, (field, value)
        assert field in last(), (field, value, last())
    # min_neighbours < rank, and its upper end per radius
    assert raw_host(lib.despeckle_params(rank=4, min_neighbours=3), rad, albedo, ids, None, out) == T.FF_ERR_INVALID_ARG and "min_neighbours" in last()
    for r in RADII:
        top = (2 * r + 1) ** 2 - 1
        assert raw_host(lib.despeckle_params(radius=r, min_neighbours=top), rad, albedo, ids, None, out) == T.FF_OK
        assert raw_host(lib.despeckle_params(radius=r, min_neighbours=top + 1), rad, albedo, ids, None, out) == T.FF_ERR_INVALID_ARG and "min_neighbours" in last()
    out[:] = 7.0
    p = lib.despeckle_params()
    for args, word in [((None, rad, albedo, ids), "params"), ((p, None, albedo, ids), "radiance_in"), ((p, rad, albedo, None), "ids"),
                       ((p, rad, None, ids), "albedo")]:
        assert raw_host(*args, None, out, w=17, h=15) == T.FF_ERR_INVALID_ARG and word in last(), (word, last())
    # without the flag no albedo is needed
    assert raw_host(lib.despeckle_params(flags=0), rad, None, ids, None, np.empty_like(rad)) == T.FF_OK
    for w, h in [(0, 15), (17, 0), (65536, 1), (1, 65536), (-1, 3)]:
        assert raw_host(p, rad, albedo, ids, None, out, w=w, h=h) == T.FF_ERR_INVALID_ARG and "size" in last()
    # overlapping buffers: the float output on each input, the bytes on an input and on the floats
    idsf = ids.view(F)
    for o, word in [(rad, "radiance_out overlaps radiance_in"), (albedo, "radiance_out overlaps albedo"), (idsf, "radiance_out overlaps ids")]:
        assert raw_host(p, rad, albedo, ids, None, o) == T.FF_ERR_INVALID_ARG and word in last(), (word, last())
    tail = rad.reshape(-1)[3:]  # (partly: it starts inside radiance_in)
    assert raw_host(p, rad, albedo, ids, None, tail) == T.FF_ERR_INVALID_ARG and "radiance_out overlaps radiance_in" in last()
    assert raw_host(p, rad, albedo, ids, albedo.view(np.uint8), out) == T.FF_ERR_INVALID_ARG and "rgb8 overlaps albedo" in last()
    assert raw_host(p, rad, albedo, ids, out.view(np.uint8), out) == T.FF_ERR_INVALID_ARG and "rgb8 overlaps radiance_out" in last()
    assert (out == 7.0).all()
    assert np.array_equal(R.bits(rad), R.bits(inputs(17, 15)[0])) and np.array_equal(ids, inputs(17, 15)[2])
    # the device entry point refuses a NULL state, and the same arguments, before it touches a device
    d = lib.load().ff_despeckle
    assert d(None, 17, 15, C.byref(p), rad.ctypes.data, albedo.ctypes.data, ids.ctypes.data, 0, None, 0, out.ctypes.data, 0, None) == T.FF_ERR_INVALID_ARG
    assert "state" in last()


@pytest.mark.parametrize("w,h", SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
def test_twin_matches_the_reference_bit_for_bit(w, h):
    rad, albedo, ids = inputs(w, h)
    changed = 0
    for r in RADII:
        for rank in RANKS:
            for flags in (FLAG, 0):
                p = lib.despeckle_params(radius=r, rank=rank, min_neighbours=max(rank, 3), flags=flags)
                rgb8, out, n = twin_matches_reference(rad, albedo if flags else None, ids, p)
                changed += n
        # min_neighbours at both ends of its range
        for rank in (1, 4):
            for mn in (rank, (2 * r + 1) ** 2 - 1):
                twin_matches_reference(rad, albedo, ids, lib.despeckle_params(radius=r, rank=rank, min_neighbours=mn))
    if w * h > 64:
        assert changed  # (the comparison is not one of copies)
    # another threshold and a floor, and only one of the outputs
    p = lib.despeckle_params(threshold=1.0, floor=0.75, radius=2)
    both = twin_matches_reference(rad, albedo, ids, p)
    only8, none, n = lib.despeckle_host(rad, {"albedo": albedo, "ids": ids}, p, want_out=False)
    assert none is None and np.array_equal(only8, both[0]) and n == both[2]
    none, only, n = lib.despeckle_host(rad, (albedo, ids), p, want_rgb8=False)
    assert none is None and np.array_equal(R.bits(only), R.bits(both[1])) and n == both[2]
    assert lib.despeckle_host(rad, (albedo, ids), p, want_rgb8=False, want_out=False) == (None, None, both[2])


def test_the_stated_consequences():
    w, h = 33, 31
    rad, albedo, ids = inputs(w, h)
    plain = np.ones_like(albedo)
    # a constant image comes back bit for bit, also with a -0 channel, for every radius and rank, at threshold 1
    flat = np.empty_like(rad)
    flat[:] = (0.7, -0.0, 3.0)
    for r in RADII:
        for rank in RANKS:
            for flags, alb in ((FLAG, plain), (0, None)):
                p = lib.despeckle_params(radius=r, rank=rank, min_neighbours=rank, threshold=1.0, flags=flags)
                rgb8, out, n = twin_matches_reference(flat, alb, ids, p)
                assert n == 0 and np.array_equal(R.bits(out), R.bits(flat)) and np.array_equal(rgb8, R.to_u8(flat))
    # a threshold whose limit overflows
    rgb8, out, n = twin_matches_reference(rad, albedo, ids, lib.despeckle_params(threshold=3.0e38))
    assert n == 0 and np.array_equal(R.bits(out), R.bits(rad)) and np.array_equal(rgb8, R.to_u8(rad))
    # with floor 0 a power of two scales the output exactly and leaves the count
    for p in (lib.despeckle_params(), lib.despeckle_params(radius=3, rank=4, min_neighbours=6, threshold=1.5, flags=0)):
        base = twin_matches_reference(rad, albedo, ids, p)
        assert base[2] > 0
        for k in (F(2.0 ** -20), F(2.0 ** 9)):
            scaled = twin_matches_reference(rad * k, albedo, ids, p)
            assert scaled[2] == base[2] and np.array_equal(R.bits(scaled[1]), R.bits(base[1] * k))
        # no pixel's l grows, clamped pixels' l falls, and no channel changes its sign
        flags = p.flags
        l_in, g = R.measure(rad, albedo, ids, flags)
        l_out, g_out = R.measure(base[1], albedo, ids, flags)
        assert np.array_equal(g, g_out) and (l_out[g >= 0] <= l_in[g >= 0]).all()
        hit = (R.bits(base[1]) != R.bits(rad)).any(axis=-1)
        assert (l_out[hit] < l_in[hit]).all() and np.array_equal(np.signbit(base[1]), np.signbit(rad))
    # a floor: nothing is pulled below it, and a floor above the image leaves it alone
    rgb8, out, n, d = reference(rad, albedo, ids, lib.despeckle_params(floor=4.0), details=True)
    assert_same(lib.despeckle_host(rad, (albedo, ids), lib.despeckle_params(floor=4.0)), (rgb8, out, n))
    assert n > 0 and (d["limit"][d["hit"]] >= F(4.0)).all() and (d["limit"][d["hit"]] == F(4.0)).any()
    assert lib.despeckle_host(rad, (albedo, ids), lib.despeckle_params(floor=3.0e38))[2] == 0


def test_a_negative_zero_channel_of_an_unclamped_pixel_stays():
    w, h = 33, 31
    rad, albedo, ids = (np.array(a) for a in inputs(w, h))
    rad[5:9, 3:9, 1] = -0.0
    rad[12, 4] = (-0.0, -0.0, -0.0)
    rgb8, out, n, d = reference(rad, albedo, ids, lib.despeckle_params(), details=True)
    assert_same(lib.despeckle_host(rad, (albedo, ids), lib.despeckle_params()), (rgb8, out, n))
    keep = ~d["hit"]
    keep[:, :] &= np.signbit(rad[..., 1])
    assert keep.sum() > 10 and (R.bits(out[..., 1][keep]) == 0x80000000).all()
    # ... and of a clamped one as well: s is positive
    assert np.array_equal(np.signbit(out), np.signbit(rad))


def l_of(out, albedo, ids, flags=FLAG):
    return R.measure(out, albedo, ids, flags)[0]


def test_planted_spikes():
    w, h = PLANT_SIZE
    rad, albedo, ids = inputs(w, h, noise=False)
    spikes = planted(w, h)
    assert len(spikes) == len(SINGLES) + 2 * len(PAIRS) + len(BLOCK) + 2 * len(SEAMS)
    spot = np.zeros((h, w), bool)
    for y, x in spikes:
        spot[y, x] = True
    # the ramp alone: the reference clamps nothing at threshold 2, for any radius and rank (the slope is that gentle)
    clean = ramp(w, h)
    assert np.array_equal(R.bits(clean[~spot]), R.bits(rad[~spot]))
    for r in RADII:
        for rank in RANKS:
            assert R.despeckle(clean, albedo, ids, radius=r, rank=rank, min_neighbours=rank)[2] == 0
    p2, p4 = lib.despeckle_params(rank=2), lib.despeckle_params(rank=4, min_neighbours=4)
    for p in (p2, p4):
        rgb8, out, n, d = reference(rad, albedo, ids, p, details=True)
        assert_same(lib.despeckle_host(rad, (albedo, ids), p), (rgb8, out, n))
        # on the reference alone: no unplanted pixel is clamped ...
        assert not (d["hit"] & ~spot).any()
        changed = (R.bits(out) != R.bits(rad)).any(axis=-1)
        # ... every unplanted pixel is returned bit for bit, and out_clamped is the number of pixels whose bits changed
        assert not (changed & ~spot).any() and n == int(changed.sum()) == int(d["hit"].sum())
        l_out = l_of(out, albedo, ids)
        gone = [yx for yx in SINGLES] + [yx for group in PAIRS for yx in group]
        if p is p4:
            gone += BLOCK
        for y, x in gone:
            assert d["hit"][y, x] and l_out[y, x] <= d["limit"][y, x], ((y, x), l_out[y, x], d["limit"][y, x])
            assert l_out[y, x] < 2.5 * l_of(clean, albedo, ids)[y, x]
        if p is p2:
            for y, x in BLOCK:  # three spiky neighbours each: the second largest is a spike
                assert not d["hit"][y, x] and np.array_equal(R.bits(out[y, x]), R.bits(rad[y, x]))


def test_every_clamped_pixel_measures_at_or_below_its_limit():
    """Step 3 lowers its factor until the output, measured again as step 1 measures, is not above the limit: a bare <= in float32,
    on the planted spikes and on every clamped pixel of the noisy images, for every radius and rank and both flag settings.  The
    bare quotient limit / l alone would leave pixels one unit in the last place above (two of the eleven planted singles and pairs
    at the defaults): some pixels must have been lowered.  None by more than 16
    steps: on radiance >= 0 the quotient, a product, two divisions and the three products and two sums of each of the two
    luminances are about a dozen roundings of at most 2^-24, and a step lowers s by at least 2^-24 of itself."""
    lowered = 0
    for (w, h), noise in ((PLANT_SIZE, False), (PLANT_SIZE, True), ((33, 31), True)):
        rad, albedo, ids = inputs(w, h, noise=noise)
        for r in RADII:
            for rank in RANKS:
                for flags in (FLAG, 0):
                    p = lib.despeckle_params(radius=r, rank=rank, min_neighbours=max(rank, 3), flags=flags)
                    alb = albedo if flags else None
                    rgb8, out, n, d = reference(rad, alb, ids, p, details=True)
                    assert_same(lib.despeckle_host(rad, (alb, ids), p), (rgb8, out, n))
                    l_out = l_of(out, alb, ids, flags)
                    hit = d["hit"]
                    assert n > 0 and (l_out[hit] <= d["limit"][hit]).all() and (l_out[hit] < d["l"][hit]).all()
                    assert d["lowered"].max() <= 16
                    lowered += int((d["lowered"] > 0).sum())
    assert lowered > 0


def test_the_neighbour_across_a_tile_seam_decides():
    """The pairs of SEAMS lie 1, 2 and 3 pixels apart across x = 32, y = 8 and the corner (64, 8): with rank 1 a spike survives
    exactly from the radius on at which its window holds the other half, with rank 2 it never does."""
    w, h = PLANT_SIZE
    rad, albedo, ids = inputs(w, h, noise=False)
    for group in SEAMS:
        (ya, xa), (yb, xb) = group
        apart = max(abs(ya - yb), abs(xa - xb))
        assert (xa < 32 <= xb or xa < 64 <= xb) or ya < 8 <= yb
        for r in RADII:
            out1 = lib.despeckle_host(rad, (albedo, ids), lib.despeckle_params(radius=r, rank=1, min_neighbours=3))[1]
            out2 = lib.despeckle_host(rad, (albedo, ids), lib.despeckle_params(radius=r, rank=2, min_neighbours=3))[1]
            for y, x in group:
                survives = np.array_equal(R.bits(out1[y, x]), R.bits(rad[y, x]))
                assert survives == (r >= apart), (group, r)
                assert not np.array_equal(R.bits(out2[y, x]), R.bits(rad[y, x]))


def test_emitter_miss_and_thin_strip_pixels_are_untouched():
    w, h = PLANT_SIZE
    rad, albedo, ids = (np.array(a) for a in inputs(w, h))
    emitter, miss, strip = ids[..., 2] == T.BXDF_EMITTER, ids[..., 0] < 0, ids[..., 0] == 3
    emitter &= ~miss
    assert emitter.sum() > 20 and miss.sum() > 100 and strip.sum() == 3
    still = emitter | miss | strip
    rad[still] *= F(1.0e5)       # every one of them a firefly
    rad[2, w // 2] *= F(1.0e3)  # ... and one of the strip far above the strip's others
    for r in RADII:
        for rank in (1, 2):
            p = lib.despeckle_params(radius=r, rank=rank)
            rgb8, out, n = twin_matches_reference(rad, albedo, ids, p)
            assert n > 0 and np.array_equal(R.bits(out[still]), R.bits(rad[still]))
    # (the strip is judged once two neighbours are enough)
    out = twin_matches_reference(rad, albedo, ids, lib.despeckle_params(rank=1, min_neighbours=2))[1]
    assert (R.bits(out[strip]) != R.bits(rad[strip])).any()
    assert np.array_equal(R.bits(out[emitter | miss]), R.bits(rad[emitter | miss]))


def test_non_finite_pixels_spoil_only_themselves():
    w, h = 33, 31
    rad, albedo, ids = (np.array(a) for a in inputs(w, h))
    spots = [(3, 4), (10, 20), (10, 21), (20, 5), (25, 30), (15, 15)]
    rad[3, 4] = (np.nan, 0.5, 0.25)
    rad[10, 20] = np.inf
    rad[10, 21] = (-np.inf, 1.0, 1.0)
    rad[20, 5] = (1.0, np.nan, np.inf)
    rad[25, 30] = (3.0e38, 3.0e38, 3.0e38)  # finite channels, but l is not once it is divided by the albedo
    albedo[25, 30] = (0.25, 0.25, 0.25)
    nan_albedo = (15, 15)
    albedo[nan_albedo] = (0.5, np.nan, 0.5)
    missed = ids.copy()
    for yx in spots:
        missed[yx] = (-1, -1, -1)
    for r in RADII:
        for rank in (1, 2, 4):
            p = lib.despeckle_params(radius=r, rank=rank, min_neighbours=max(rank, 3))
            rgb8, out, n = twin_matches_reference(rad, albedo, ids, p)
            for yx in spots:
                assert np.array_equal(R.bits(out[yx]), R.bits(rad[yx]))  # copied through
            # their neighbours skip them: the output is the one their ids would give as misses
            assert_same((rgb8, out, n), lib.despeckle_host(rad, (albedo, missed), p))
    # without the flag the albedo is not read: the pixel with the NaN albedo counts like any other
    p = lib.despeckle_params(flags=0)
    rad[nan_albedo] *= F(1.0e4)
    out = twin_matches_reference(rad, None, ids, p)[1]
    assert (R.bits(out[nan_albedo]) != R.bits(rad[nan_albedo])).any()
