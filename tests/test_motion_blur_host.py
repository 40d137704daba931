"""ff_motion_blur on the host side: exports, defaults, every argument check (all before any device work), and the host twin
ff_motion_blur_host - the kernels' per-pixel functions compiled for the host - bit for bit against the numpy float32 reference
(tests/motion_blur_ref.py) over sizes, tile edges, tap counts and shutters, and the operator's properties: identities, locality,
the tie rule, non-finite input, and what it is for (closer to the shutter average than the unblurred frame)."""
import ctypes as C
import re
import os

import numpy as np
import pytest

from gpupathtracer_amd import lib
from gpupathtracer_amd import types as T
import motion_blur_ref as R
from motion_blur_cases import SIZES, assert_same, inputs, params_of

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RADII = [1, 2, 16, 64]
MORE_RADII = [3, 5, 8, 9]  # the device packs tiles of up to 8 x 8 pixels by lane groups of 16, 32 and 64: both sides of that edge
SAMPLES = [1, 2, 15, 64]
SHUTTERS = [0.25, 1.0, 4.0]


def twin_matches_reference(rad, motion, depth, p):
    got = lib.motion_blur_host(rad, motion, depth, p)
    assert_same(got, R.motion_blur(rad, motion, depth, **params_of(p)))
    return got


def test_new_entry_points_are_exported_and_declared(ff):
    handle = ff.load()
    header = open(os.path.join(ROOT, "include", "firefly", "ff_api.h")).read()
    declared = set(re.findall(r"FF_API\s+[\w\s\*]+?\b(ff_\w+)\s*\(", header))
    for name in ("ff_motion_blur_params_init", "ff_motion_blur", "ff_motion_blur_host"):
        assert name in ff.EXPORTS and name in declared and hasattr(handle, name), name


def test_motion_blur_params_defaults():
    p = lib.motion_blur_params()
    assert p.shutter == F(0.5) and p.max_radius == 16 and p.samples == 15 and p.depth_extent == F(0.1) and p.flags == 0 and p.reserved == 0
    assert C.sizeof(T.FfMotionBlurParams) == T.MOTION_BLUR_PARAMS_BYTES == 24
    q = lib.motion_blur_params(shutter=1.0, samples=7)
    assert q.shutter == 1.0 and q.samples == 7
    with pytest.raises(TypeError):
        lib.motion_blur_params(radius=3)


@pytest.mark.parametrize("w,h", SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
def test_twin_matches_the_reference_bit_for_bit(w, h):
    rad, motion, depth = inputs(w, h)
    blurred = 0
    for k in RADII:
        for S in SAMPLES:
            for shutter in SHUTTERS:
                out = twin_matches_reference(rad, motion, depth, lib.motion_blur_params(shutter=shutter, max_radius=k, samples=S))[1]
                blurred += int((R.bits(out) != R.bits(rad)).any())
    for k in MORE_RADII:
        twin_matches_reference(rad, motion, depth, lib.motion_blur_params(shutter=1.0, max_radius=k))
    if w * h > 1:
        assert blurred  # (the comparison is not one of copies)
    # another depth_extent, and only one of the outputs
    p = lib.motion_blur_params(shutter=1.0, depth_extent=2.5)
    both = twin_matches_reference(rad, motion, depth, p)
    only8, none = lib.motion_blur_host(rad, motion, depth, p, want_out=False)
    assert none is None and np.array_equal(only8, both[0])
    none, only = lib.motion_blur_host(rad, motion, depth, p, want_rgb8=False)
    assert none is None and np.array_equal(R.bits(only), R.bits(both[1]))


def test_identities_bit_for_bit():
    w, h = 33, 31
    rad, motion, depth = inputs(w, h)
    dirty = rad.copy()
    dirty[3, 4] = (np.nan, 0.5, 0.25)
    dirty[10, 20] = np.inf
    dirty[30, 32] = (-np.inf, np.nan, 1.0)
    for p in (lib.motion_blur_params(), lib.motion_blur_params(shutter=4.0, max_radius=2, samples=64)):
        # all-zero motion, also with NaN and +-Inf pixels in the image
        for image in (rad, dirty):
            rgb8, out = lib.motion_blur_host(image, np.zeros_like(motion), depth, p)
            assert np.array_equal(R.bits(out), R.bits(image)) and np.array_equal(rgb8, R.to_u8(image))
        # a closed shutter
        p0 = lib.motion_blur_params(**dict(params_of(p), shutter=0.0))
        for image in (rad, dirty):
            rgb8, out = lib.motion_blur_host(image, motion, depth, p0)
            assert np.array_equal(R.bits(out), R.bits(image)) and np.array_equal(rgb8, R.to_u8(image))
        # a constant colour under any motion
        flat = np.empty_like(rad)
        flat[:] = (0.7, 0.05, 3.0)
        p1 = lib.motion_blur_params(**dict(params_of(p), shutter=1.0))
        rgb8, out = lib.motion_blur_host(flat, motion, depth, p1)
        assert np.array_equal(R.bits(out), R.bits(flat)) and np.array_equal(rgb8, R.to_u8(flat))
        # ... also one with a -0 channel: where nothing is added the centre's bits come back, not -0 + 0 = +0
        flat[..., 1] = -0.0
        rgb8, out = twin_matches_reference(flat, motion, depth, p1)
        assert np.array_equal(R.bits(out), R.bits(flat)) and (R.bits(out[..., 1]) == 0x80000000).all()


def test_only_the_tiles_around_a_moving_block_change():
    w, h, k = 96, 48, 16
    rad, _, depth = inputs(w, h)
    motion = np.zeros((h, w, 2), np.float32)
    motion[20:24, 40:44] = (12.0, 0.0)  # tile (2, 1)
    p = lib.motion_blur_params(shutter=1.0, max_radius=k)
    rgb8, out = twin_matches_reference(rad, motion, depth, p)
    changed = (R.bits(out) != R.bits(rad)).any(axis=-1)
    near = np.zeros((h, w), bool)
    near[0:48, 16:64] = True  # the 3 x 3 tiles around tile (2, 1)
    assert not changed[~near].any()
    assert np.array_equal(rgb8[~near], R.to_u8(rad)[~near])
    outside = changed.copy()
    outside[20:24, 40:44] = False
    assert outside[20:24, 40 - k:44 + k].any()  # the block smears over its neighbours along x


def test_ties_go_to_the_first_pixel_in_row_major_order():
    w, h, k = 32, 16, 16
    rad, _, depth = inputs(w, h)
    first, second = (2, 9), (5, 3)  # (row, column), both in tile (0, 0); (2, 9) comes first
    outs = []
    for a, b in (((12.0, 0.0), (0.0, 12.0)), ((0.0, 12.0), (12.0, 0.0))):
        motion = np.zeros((h, w, 2), np.float32)
        motion[first], motion[second] = a, b
        p = lib.motion_blur_params(shutter=1.0, max_radius=k)
        v, l, _ = R.pack(motion, depth, 1.0, k)
        tmax = R.tile_max(v, l, k)
        assert tmax[0, 0].tolist() == [a[0] * 0.5, a[1] * 0.5, 6.0]
        outs.append(twin_matches_reference(rad, motion, depth, p)[1])
    assert not np.array_equal(R.bits(outs[0]), R.bits(outs[1]))  # (the direction that wins decides where the taps lie)
    # ... and among tiles: equal speeds in tiles (0, 0) and (1, 0), the first tile decides for both
    motion = np.zeros((h, w, 2), np.float32)
    motion[4, 4], motion[4, 20] = (0.0, 12.0), (12.0, 0.0)
    v, l, _ = R.pack(motion, depth, 1.0, k)
    nmax = R.neighbour_max(R.tile_max(v, l, k))
    assert nmax[0, 0].tolist() == nmax[0, 1].tolist() == [0.0, 6.0, 6.0]
    twin_matches_reference(rad, motion, depth, lib.motion_blur_params(shutter=1.0, max_radius=k))


def test_non_finite_pixels_spoil_only_themselves():
    w, h = 64, 64
    rad, _, depth = inputs(w, h)
    motion = np.zeros((h, w, 2), np.float32)
    motion[16:48, 8:56] = (20.0, -6.0)
    spots = [(30, 30), (33, 27)]
    dirty, black = rad.copy(), rad.copy()
    dirty[spots[0]] = (np.nan, 0.5, 0.25)
    dirty[spots[1]] = np.inf
    mask = np.ones((h, w), bool)
    for s in spots:
        black[s] = 0.0
        mask[s] = False
    p = lib.motion_blur_params(shutter=1.0)
    rgb8, out = twin_matches_reference(dirty, motion, depth, p)
    assert np.isfinite(out[mask]).all()
    for s in spots:
        assert np.array_equal(R.bits(out[s]), R.bits(dirty[s]))  # copied through
    want8, want = R.motion_blur(black, motion, depth, exclude=~mask, **params_of(p))
    assert np.array_equal(R.bits(out[mask]), R.bits(want[mask])) and np.array_equal(rgb8[mask], want8[mask])
    clean = lib.motion_blur_host(black, motion, depth, p)[1]
    assert (R.bits(clean[mask]) != R.bits(out[mask])).any()  # (the two pixels do lie under taps: leaving them out is seen)
    # non-finite motion is no motion, non-finite depth is a miss
    bad_motion, as_zero = motion.copy(), motion.copy()
    bad_depth, as_miss = depth.copy(), depth.copy()
    for (y, x), m in zip([(20, 20), (21, 40), (40, 12)], [(np.nan, 3.0), (np.inf, 0.0), (5.0, -np.inf)]):
        bad_motion[y, x] = m
        as_zero[y, x] = 0.0
    for (y, x), z in zip([(25, 25), (26, 41), (41, 13), (42, 14)], [np.nan, np.inf, -np.inf, -2.0]):
        bad_depth[y, x] = z
        as_miss[y, x] = 0.0
    assert_same(twin_matches_reference(rad, bad_motion, bad_depth, p), lib.motion_blur_host(rad, as_zero, as_miss, p))


def shutter_average_case():
    """A step edge under uniform motion, and the step box-filtered over the 16 px it moves while the shutter is open."""
    w, h, k = 128, 32, 16
    rad = np.zeros((h, w, 3), np.float32)
    rad[:, w // 2:] = 1.0
    motion = np.zeros((h, w, 2), np.float32)
    motion[..., 0] = 16.0
    depth = np.full((h, w), 2.0, np.float32)
    box = np.convolve(rad[0, :, 0].astype(np.float64), np.full(17, 1.0 / 16.0) * np.r_[0.5, np.ones(15), 0.5], mode="same")
    truth = np.broadcast_to(box[None, :, None], rad.shape)
    return rad, motion, depth, truth, k


def mse_ratio(out, rad, truth, k):
    cols = slice(k, rad.shape[1] - k)
    blurred = float(((out[:, cols].astype(np.float64) - truth[:, cols]) ** 2).mean())
    plain = float(((rad[:, cols].astype(np.float64) - truth[:, cols]) ** 2).mean())
    return blurred, plain


def test_the_blur_is_closer_to_the_shutter_average_than_the_frame():
    """What the operator is for.  Measured: MSE 0.000174 against the unblurred frame's 0.0138 (ratio 0.0126)."""
    rad, motion, depth, truth, k = shutter_average_case()
    out = twin_matches_reference(rad, motion, depth, lib.motion_blur_params(shutter=1.0, max_radius=k))[1]
    blurred, plain = mse_ratio(out, rad, truth, k)
    print(f"MSE blurred {blurred:.6g}, unblurred {plain:.6g}, ratio {blurred / plain:.4g}")
    assert blurred < plain


@pytest.mark.parametrize("entry", ["ff_motion_blur", "ff_motion_blur_host"])
def test_invalid_arguments_are_refused_before_any_device_work(ff, entry):
    handle = ff.load()
    state = C.c_void_p(0x1)  # never dereferenced: every check below fails before the state is used
    w, h = 8, 4
    rad = np.zeros((h, w, 3), np.float32)
    motion = np.zeros((h, w, 2), np.float32)
    depth = np.zeros((h, w), np.float32)
    out = np.full((h, w, 3), 7.0, np.float32)
    rgb8 = np.full((h, w, 3), 7, np.uint8)
    ptr = lambda a: a.ctypes.data if a is not None else None  # noqa: E731

    def call(p, w=w, h=h, rad=rad, motion=motion, depth=depth, rgb8=rgb8, out=out, state=state):
        pp = C.byref(p) if p is not None else None
        if entry == "ff_motion_blur":
            return handle.ff_motion_blur(state, w, h, pp, ptr(rad), ptr(motion), ptr(depth), 0, ptr(rgb8), 0, ptr(out), 0)
        return handle.ff_motion_blur_host(w, h, pp, ptr(rad), ptr(motion), ptr(depth), ptr(rgb8), ptr(out))

    def refused(word, *args, **kw):
        assert call(*args, **kw) == T.FF_ERR_INVALID_ARG
        assert word in handle.ff_last_error().decode(), handle.ff_last_error()
    good = lib.motion_blur_params()
    nan, inf = float("nan"), float("inf")
    for field, values in [("shutter", (-0.1, 4.5, nan, inf)), ("max_radius", (0, 65, -3)), ("samples", (0, 65, -1)),
                          ("depth_extent", (0.0, -1.0, nan, inf)), ("flags", (1, -1)), ("reserved", (1,))]:
        for value in values:
            refused(field, lib.motion_blur_params(**{field: value}))
    refused("params", None)
    if entry == "ff_motion_blur":
        refused("state", good, state=None)
    refused("radiance_in", good, rad=None)
    refused("motion", good, motion=None)
    refused("depth", good, depth=None)
    for bw, bh in [(0, 4), (8, 0), (-1, 4), (8, 70000), (65536, 1)]:
        refused("size", good, bw, bh)
    # an output on top of an input, or overlapping it
    refused("radiance_out overlaps radiance_in", good, out=rad)
    big = np.zeros(h * w * 3 + 8, np.float32)
    refused("radiance_out overlaps radiance_in", good, rad=big[:h * w * 3].reshape(h, w, 3), out=big[8:].reshape(h, w, 3))
    refused("radiance_out overlaps motion", good, out=big[:h * w * 3].reshape(h, w, 3), motion=big[h * w:h * w * 3].reshape(h, w, 2))
    refused("rgb8 overlaps depth", good, rgb8=depth.view(np.uint8))
    # the two outputs on each other
    both = np.zeros(h * w * 3 + 4, np.float32)
    refused("rgb8 overlaps radiance_out", good, rgb8=both[h * w * 3 - 4:].view(np.uint8), out=both[:h * w * 3].reshape(h, w, 3))
    assert (out == 7.0).all() and (rgb8 == 7).all()
    # the edges of the ranges are accepted (host twin: it needs no state)
    if entry == "ff_motion_blur_host":
        for edge in (dict(shutter=0.0), dict(shutter=4.0), dict(max_radius=1, samples=1), dict(max_radius=64, samples=64)):
            assert call(lib.motion_blur_params(**edge), rgb8=None) == T.FF_OK
