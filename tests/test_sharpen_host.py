"""ff_sharpen on the host side: exports, defaults, every argument check (all before any device work), the host twin ff_sharpen_host -
the kernel's per-pixel functions compiled for the host - bit for bit against the numpy float32 restatement (tests/sharpen_ref.py)
over sizes, both flag settings and four strengths, the consequences the header states, the step edges, and a count of every branch
the operator has."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from gpupathtracer_amd import lib
from gpupathtracer_amd import types as T
import sharpen_ref as R
from sharpen_cases import (BLACK, CHECKER, DIAGONAL, FLAG_SETTINGS, H_EDGE, ISOLUMINANT, LIT, PLANT_SIZE, SATURATED, SEAM_EDGES, SEAM_UNUSABLE, SIZES,
                           STRENGTHS, UNUSABLE, USABLE_ODDITIES, V_EDGE, assert_same, corners, cross, inputs, reference)

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAG = T.SHARPEN_NOISE_AWARE


def twin_matches_reference(rad, p):
    got = lib.sharpen_host(rad, p)
    assert_same(got, reference(rad, p))
    return got


def test_new_entry_points_are_exported_and_declared(ff):
    handle = ff.load()
    header = open(os.path.join(ROOT, "include", "firefly", "ff_api.h")).read()
    declared = set(re.findall(r"FF_API\s+[\w\s\*]+?\b(ff_\w+)\s*\(", header))
    for name in ("ff_sharpen_params_init", "ff_sharpen", "ff_sharpen_host"):
        assert name in ff.EXPORTS and name in declared and hasattr(handle, name), name


def test_sharpen_params_defaults_and_size():
    p = lib.sharpen_params()
    assert (p.strength, p.flags, p.reserved) == (0.5, FLAG, 0)
    assert C.sizeof(T.FfSharpenParams) == T.SHARPEN_PARAMS_BYTES == 12
    types_h = open(os.path.join(ROOT, "include", "firefly", "ff_types.h")).read()
    assert "static_assert(sizeof(FfSharpenParams) == 12" in types_h and "_Static_assert(sizeof(FfSharpenParams) == 12" in types_h
    assert re.search(r"#define\s+FF_SHARPEN_NOISE_AWARE\s+1\b", types_h)
    q = lib.sharpen_params(strength=1.0, flags=0)
    assert q.strength == 1.0 and q.flags == 0
    with pytest.raises(TypeError):
        lib.sharpen_params(radius=3)
    # the restatement's constants are the header's
    api_h = open(os.path.join(ROOT, "include", "firefly", "ff_api.h")).read()
    assert "LIMIT = 0.1875f, CAP = 0.99999988f (1 - 2^-23), MAXC = 8388608.0f (2^23)" in api_h


def raw_host(p, rad, rgb8=None, out=None, w=None, h=None):
    ptr = lambda a: a.ctypes.data if a is not None else None  # noqa: E731
    hh, ww = rad.shape[:2] if rad is not None else (9, 17)
    return lib.load().ff_sharpen_host(ww if w is None else w, hh if h is None else h, C.byref(p) if p is not None else None, ptr(rad), ptr(rgb8), ptr(out))


def test_every_refused_argument_names_its_field():
    rad = np.array(inputs(17, 15))
    out = np.full(rad.shape, 7.0, F)
    last = lambda: lib.load().ff_last_error().decode()  # noqa: E731
    nan, inf = float("nan"), float("inf")
    cases = [("strength", -0.25), ("strength", 1.5), ("strength", nan), ("strength", inf), ("strength", -inf), ("flags", 2), ("flags", 3),
             ("flags", 0x80000001), ("reserved", 1)]
    for field, value in cases:
        assert raw_host(lib.sharpen_params(**{field: value}), rad, None, out) == T.FF_ERR_INVALID_ARG, (field, value)
        assert field in last(), (field, value, last())
    for value in (0.0, -0.0, 1.0):  # (both ends are allowed)
        assert raw_host(lib.sharpen_params(strength=value), rad, None, out) == T.FF_OK
    out[:] = 7.0
    p = lib.sharpen_params()
    for args, word in [((None, rad), "params"), ((p, None), "radiance_in")]:
        assert raw_host(*args, None, out, w=17, h=15) == T.FF_ERR_INVALID_ARG and word in last(), (word, last())
    for w, h in [(0, 15), (17, 0), (65536, 1), (1, 65536), (-1, 3)]:
        assert raw_host(p, rad, None, out, w=w, h=h) == T.FF_ERR_INVALID_ARG and "size" in last()
    # overlapping buffers: the float output on the input (in place, and partly), the bytes on the input and on the floats
    assert raw_host(p, rad, None, rad) == T.FF_ERR_INVALID_ARG and "radiance_out overlaps radiance_in" in last()
    tail = rad.reshape(-1)[3:]  # (it starts inside radiance_in)
    assert raw_host(p, rad, None, tail) == T.FF_ERR_INVALID_ARG and "radiance_out overlaps radiance_in" in last()
    assert raw_host(p, rad, rad.view(np.uint8), out) == T.FF_ERR_INVALID_ARG and "rgb8 overlaps radiance_in" in last()
    spare = np.array(rad)  # (a 1 x 1 call reads 12 bytes: bytes further on in the same array are no overlap)
    assert raw_host(p, spare, spare.view(np.uint8).reshape(-1)[-8:], out, w=1, h=1) == T.FF_OK
    assert raw_host(p, rad, out.view(np.uint8), out) == T.FF_ERR_INVALID_ARG and "rgb8 overlaps radiance_out" in last()
    out[:] = 7.0
    assert raw_host(p, rad, out.view(np.uint8).reshape(-1)[-3:], out, w=1, h=1) == T.FF_OK
    out[:] = 7.0
    assert raw_host(lib.sharpen_params(strength=2.0), rad, None, out) == T.FF_ERR_INVALID_ARG and (out == 7.0).all()
    assert np.array_equal(R.bits(rad), R.bits(inputs(17, 15)))
    # the device entry point refuses a NULL state, and the same arguments, before it touches a device
    d = lib.load().ff_sharpen
    assert d(None, 17, 15, C.byref(p), rad.ctypes.data, 0, None, 0, out.ctypes.data, 0) == T.FF_ERR_INVALID_ARG
    assert "state" in last()


@pytest.mark.parametrize("w,h", SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
def test_twin_matches_the_reference_bit_for_bit(w, h):
    rad = inputs(w, h)
    changed = 0
    for flags in FLAG_SETTINGS:
        for strength in STRENGTHS:
            rgb8, out = twin_matches_reference(rad, lib.sharpen_params(strength=strength, flags=flags))
            changed += int((R.bits(out) != R.bits(rad)).sum())
    if w * h > 4:
        assert changed  # (the comparison is not one of copies)
    # only one of the outputs
    p = lib.sharpen_params(strength=0.75)
    both = twin_matches_reference(rad, p)
    only8, none = lib.sharpen_host(rad, p, want_out=False)
    assert none is None and np.array_equal(only8, both[0])
    none, only = lib.sharpen_host(rad, p, want_rgb8=False)
    assert none is None and np.array_equal(R.bits(only), R.bits(both[1]))
    assert lib.sharpen_host(rad, p, want_rgb8=False, want_out=False) == (None, None)


def test_the_stated_consequences():
    w, h = PLANT_SIZE
    rad = inputs(w, h)
    # strength 0 returns the input bit for bit, NaN, Inf and -0 included
    assert not np.isfinite(rad).all() and (R.bits(rad) == 0x80000000).any()
    for flags in FLAG_SETTINGS:
        for zero in (0.0, -0.0):
            rgb8, out = twin_matches_reference(rad, lib.sharpen_params(strength=zero, flags=flags))
            assert np.array_equal(R.bits(out), R.bits(rad)) and np.array_equal(rgb8, R.to_u8(rad))
    # a constant image, also with a -0 channel, and a 1 x 1 image
    flat = np.empty((9, 33, 3), F)
    flat[:] = (0.7, -0.0, 3.0)
    one = np.array([[[0.25, 1.0e5, 0.0]]], F)
    for img in (flat, one, np.zeros((5, 5, 3), F)):
        for flags in FLAG_SETTINGS:
            rgb8, out = twin_matches_reference(img, lib.sharpen_params(strength=1.0, flags=flags))
            assert np.array_equal(R.bits(out), R.bits(img)) and np.array_equal(rgb8, R.to_u8(img))
    for flags in FLAG_SETTINGS:
        for strength in STRENGTHS[1:]:
            p = lib.sharpen_params(strength=strength, flags=flags)
            rgb8, out, d = reference(rad, p, details=True)
            assert_same(lib.sharpen_host(rad, p), (rgb8, out))
            # every pixel with an unusable pixel in its cross is copied through, the unusable pixel itself too
            spoiled = ~d["all_usable"]
            assert (~d["usable"]).sum() == len(UNUSABLE) + len(SEAM_UNUSABLE)
            assert spoiled.sum() > 4 * (~d["usable"]).sum() and np.array_equal(R.bits(out[spoiled]), R.bits(rad[spoiled]))
            # ... and nothing further is spoiled: what changed is finite, >= 0 and at most CAP * 2^23
            hit = (R.bits(out) != R.bits(rad)).any(axis=-1)
            assert hit.sum() > w * h // 2 and not (hit & ~d["active"]).any()
            top = F(R.CAP * R.MAXC)
            assert np.isfinite(out[d["active"]]).all() and (out[d["active"]] >= 0).all() and (out[d["active"]] <= top).all()
            assert not np.signbit(out[d["active"]]).any()
            assert np.array_equal(rgb8, R.to_u8(out))
    # the usable oddities take part: a -0 channel, a pixel of three -0, a pixel at exactly MAXC
    out = lib.sharpen_host(rad, lib.sharpen_params(strength=1.0))[1]
    d = reference(rad, lib.sharpen_params(strength=1.0), details=True)[2]
    for yx in USABLE_ODDITIES:
        assert d["usable"][yx] and d["active"][yx] and not np.signbit(out[yx]).any()


def test_an_unusable_pixel_spoils_its_cross_and_no_more():
    """Also across the seams of the kernel's tiles: the four cross neighbours of every planted unusable pixel come back bit for bit,
    its diagonal neighbours - the corners the apron leaves out - are sharpened."""
    w, h = PLANT_SIZE
    rad = inputs(w, h)
    for flags in FLAG_SETTINGS:
        p = lib.sharpen_params(strength=1.0, flags=flags)
        out = twin_matches_reference(rad, p)[1]
        for y, x in list(UNUSABLE) + SEAM_UNUSABLE:
            assert np.array_equal(R.bits(out[y, x]), R.bits(rad[y, x]))
            assert len(cross(y, x, w, h)) == 4 and len(corners(y, x, w, h)) == 4
            for q in cross(y, x, w, h):
                assert np.array_equal(R.bits(out[q]), R.bits(rad[q])), ((y, x), q)
            for q in corners(y, x, w, h):
                assert not np.array_equal(R.bits(out[q]), R.bits(rad[q])), ((y, x), q)
    assert {(y, x) for y, x in SEAM_UNUSABLE if x in (31, 32)} and {(y, x) for y, x in SEAM_UNUSABLE if y in (7, 8)}
    # the same pixels made usable: their neighbours are sharpened, so it was the unusable pixel that stopped them
    clean = np.array(rad)
    for y, x in SEAM_UNUSABLE:
        clean[y, x] = (0.5, 0.4, 0.3)
    out = twin_matches_reference(clean, lib.sharpen_params(strength=1.0))[1]
    for y, x in SEAM_UNUSABLE:
        for q in cross(y, x, w, h):
            assert not np.array_equal(R.bits(out[q]), R.bits(clean[q])), ((y, x), q)


def edge_pairs():
    """((y, xa), (y, xb)) or ((ya, x), (yb, x)): adjacent pixels on the two sides of every planted step edge, away from the
    rectangles' borders."""
    pairs = []
    y0, y1, x0, x1 = V_EDGE
    pairs += [((y, (x0 + x1) // 2 - 1), (y, (x0 + x1) // 2)) for y in range(y0 + 1, y1 - 1)]
    y0, y1, x0, x1 = H_EDGE
    pairs += [(((y0 + y1) // 2 - 1, x), ((y0 + y1) // 2, x)) for x in range(x0 + 1, x1 - 1)]
    y0, y1, x0, x1 = DIAGONAL
    pairs += [((y, y + 10), (y, y + 11)) for y in range(y0 + 1, y1 - 1) if x0 + 1 <= y + 10 and y + 11 < x1 - 1]
    for y0, y1, x0, x1, axis, at in SEAM_EDGES:
        if axis == "x":
            pairs += [((y, at - 1), (y, at)) for y in range(y0 + 1, y1 - 1)]
        else:
            pairs += [((at - 1, x), (at, x)) for x in range(x0 + 1, x1 - 1)]
    return pairs


def test_step_edges_are_steepened():
    w, h = PLANT_SIZE
    rad = inputs(w, h)
    pairs = edge_pairs()
    assert len(pairs) > 40
    for flags in FLAG_SETTINGS:
        for strength in STRENGTHS[1:]:
            out = twin_matches_reference(rad, lib.sharpen_params(strength=strength, flags=flags))[1]
            for a, b in pairs:
                assert (rad[a] < rad[b]).all()
                assert (R.bits(out[a]) != R.bits(rad[a])).any() and (R.bits(out[b]) != R.bits(rad[b])).any(), (a, b)
                assert (np.abs(out[b] - out[a]) >= np.abs(rad[b] - rad[a])).all(), (a, b, out[a], out[b])
                assert (out[a] <= rad[a]).all() and (out[b] >= rad[b]).all()
            # ... and the flat insides of the rectangles are left alone (a constant neighbourhood)
            for y0, y1, x0, x1 in (V_EDGE, H_EDGE):
                inner = (slice(y0 + 1, y0 + 3), slice(x0 + 1, x0 + 3))
                assert np.array_equal(R.bits(out[inner]), R.bits(rad[inner]))


def test_every_branch_is_taken():
    """Counted on the restatement, which the twin matches bit for bit on the same image and parameters."""
    w, h = PLANT_SIZE
    rad = inputs(w, h)
    p = lib.sharpen_params(strength=1.0)
    rgb8, out, d = reference(rad, p, details=True)
    assert_same(lib.sharpen_host(rad, p), (rgb8, out))
    judged, active = d["judged"], d["active"]
    black_channel = (d["mx"] == 0) & judged[..., None]
    clamp_low = (d["raw"] < 0) & active[..., None]
    clamp_high = (d["raw"] > R.CAP) & active[..., None]
    flat_luminance = (d["range"] == 0) & judged
    no_room = judged & (d["lobe"] == 0)
    counts = dict(mx_is_0=int(black_channel.sum()), clamp_to_0=int(clamp_low.sum()), clamp_to_cap=int(clamp_high.sum()),
                  range_is_0=int(flat_luminance.sum()), lobe_is_0=int(no_room.sum()), same=int((d["all_usable"] & d["same"]).sum()),
                  unusable=int((~d["all_usable"]).sum()))
    print(counts)
    for name, n in counts.items():
        assert n > 0, name
    # where each comes from: the saturated region and the lit pixel in the black one; the checker's dark pixels; the spikes;
    # the isoluminant region; the neighbours of the lit pixel
    y0, y1, x0, x1 = SATURATED
    assert black_channel[y0 + 1:y1 - 1, x0 + 1:x1 - 1, 1:].all() and active[y0 + 1:y1 - 1, x0 + 1:x1 - 1].any()
    assert black_channel[LIT].all() and active[LIT] and (out[LIT] >= rad[LIT]).all()
    y0, y1, x0, x1 = CHECKER
    assert clamp_low[y0 + 1:y1 - 1, x0 + 1:x1 - 1].any()
    y0, y1, x0, x1 = ISOLUMINANT
    assert flat_luminance[y0 + 1:y1 - 1, x0 + 1:x1 - 1].all()
    for q in cross(*LIT, w, h):
        assert no_room[q] and np.array_equal(R.bits(out[q]), R.bits(rad[q]))
    y0, y1, x0, x1 = BLACK
    assert d["same"][y0 + 1:y0 + 3, x0 + 1:x0 + 3].all()
    # a pixel clamped to CAP comes back as CAP / (1 - CAP) in its largest channel
    peak = clamp_high.any(axis=-1)
    assert (out[peak].max(axis=-1) == F(R.CAP / (F(1.0) - R.CAP))).all()
    # under the flag a lone outlier gets half the lobe of the same pixel without it
    d0 = reference(rad, lib.sharpen_params(strength=1.0, flags=0), details=True)[2]
    y0, y1, x0, x1 = CHECKER
    inner = (slice(y0 + 1, y1 - 1), slice(x0 + 1, x1 - 1))
    assert (d0["lobe"][inner] == -R.LIMIT).all() and np.allclose(d["lobe"][inner], -0.5 * R.LIMIT, rtol=1.0e-6, atol=0.0)
