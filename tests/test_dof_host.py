"""ff_depth_of_field on the host side: exports, defaults, every argument check (all before any device work), the host twin
ff_depth_of_field_host - the kernels' per-pixel functions compiled for the host - bit for bit against the numpy float32 reference
(tests/dof_ref.py) over sizes, tile edges and tap grids, the operator's identities, and ff_dof_params_from_camera against the rays
of the in-path thin lens."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from gpupathtracer_amd import lib, scenes
from gpupathtracer_amd import types as T
import dof_ref as R
from dof_cases import DEFAULTS, KG, SIZES, assert_same, camera, inputs, reference, vec

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def twin_matches_reference(rad, pos, depth, cam, p, **kw):
    got = lib.depth_of_field_host(rad, (pos, depth), cam, p)
    assert_same(got, reference(rad, pos, depth, cam, p))
    return got


def test_new_entry_points_are_exported_and_declared(ff):
    handle = ff.load()
    header = open(os.path.join(ROOT, "include", "firefly", "ff_api.h")).read()
    declared = set(re.findall(r"FF_API\s+[\w\s\*]+?\b(ff_\w+)\s*\(", header))
    for name in ("ff_dof_params_init", "ff_dof_params_from_camera", "ff_depth_of_field", "ff_depth_of_field_host"):
        assert name in ff.EXPORTS and name in declared and hasattr(handle, name), name


def test_dof_params_defaults_and_size():
    p = lib.dof_params()
    assert p.focus_distance == F(1) and p.coc_scale == 0 and p.max_radius == 16 and p.grid == 4 and p.depth_extent == F(0.1)
    assert p.flags == 0 and list(p.reserved) == [0, 0]
    assert C.sizeof(T.FfDofParams) == T.DOF_PARAMS_BYTES == 32
    types_h = open(os.path.join(ROOT, "include", "firefly", "ff_types.h")).read()
    assert "static_assert(sizeof(FfDofParams) == 32" in types_h and "_Static_assert(sizeof(FfDofParams) == 32" in types_h
    q = lib.dof_params(coc_scale=3.0, grid=7)
    assert q.coc_scale == 3.0 and q.grid == 7
    with pytest.raises(TypeError):
        lib.dof_params(radius=3)


@pytest.mark.parametrize("w,h", SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
def test_twin_matches_the_reference_bit_for_bit(w, h):
    rad, pos, depth = inputs(w, h)
    cam = camera(w, h)
    blurred = 0
    for k, g in KG:
        out = twin_matches_reference(rad, pos, depth, cam, lib.dof_params(max_radius=k, grid=g, **DEFAULTS))[1]
        blurred += int((R.bits(out) != R.bits(rad)).any())
    if w * h > 1:
        assert blurred  # (the comparison is not one of copies)
    # another depth_extent and focus, and only one of the outputs
    p = lib.dof_params(focus_distance=0.75, coc_scale=7.5, depth_extent=2.5)
    both = twin_matches_reference(rad, pos, depth, cam, p)
    only8, none = lib.depth_of_field_host(rad, (pos, depth), cam, p, want_out=False)
    assert none is None and np.array_equal(only8, both[0])
    none, only = lib.depth_of_field_host(rad, {"position": pos, "depth": depth}, cam, p, want_rgb8=False)
    assert none is None and np.array_equal(R.bits(only), R.bits(both[1]))


def test_the_inputs_span_focus_blur_and_the_clamp():
    rad, pos, depth = inputs(64, 64)
    cam = camera(64, 64)
    l, zk = R.pack(pos, depth, vec(cam.m_position), vec(cam.m_forward), 2.0, 20.0, 16)
    assert (l < 0.5).any() and ((l > 0.5) & (l < 16)).any() and (l == 16).any()
    assert 0.15 < (zk == R.FLT_MAX).mean() < 0.25 and (l[zk == R.FLT_MAX] == F(10)).all()  # a miss lies at infinity: 20 * |1/2 - 0|


def test_identities_bit_for_bit():
    w, h = 33, 31
    rad, pos, depth = inputs(w, h)
    cam = camera(w, h)
    dirty = rad.copy()
    dirty[3, 4] = (np.nan, 0.5, 0.25)
    dirty[10, 20] = np.inf
    dirty[30, 32] = (-np.inf, np.nan, 1.0)
    for p in (lib.dof_params(**DEFAULTS), lib.dof_params(max_radius=2, grid=8, **DEFAULTS)):
        fields = {f: getattr(p, f) for f in ("focus_distance", "max_radius", "grid", "depth_extent")}
        # coc_scale 0, also with NaN and +-Inf pixels in the image
        p0 = lib.dof_params(coc_scale=0.0, **fields)
        for image in (rad, dirty):
            rgb8, out = lib.depth_of_field_host(image, (pos, depth), cam, p0)
            assert np.array_equal(R.bits(out), R.bits(image)) and np.array_equal(rgb8, R.to_u8(image))
        # everything in focus: a wall at the focus distance (and a radius below half a pixel beside it)
        wall = np.zeros_like(pos)
        wall[..., 2] = -2.0
        wall[:, w // 2:, 2] = -2.05  # l = 20 * |1/2 - 1/2.05| = 0.24
        for image in (rad, dirty):
            rgb8, out = lib.depth_of_field_host(image, (wall, np.full((h, w), 2.0, F)), cam, p)
            assert np.array_equal(R.bits(out), R.bits(image)) and np.array_equal(rgb8, R.to_u8(image))
        # a constant colour under any blur
        flat = np.empty_like(rad)
        flat[:] = (0.7, 0.05, 3.0)
        rgb8, out = lib.depth_of_field_host(flat, (pos, depth), cam, p)
        assert np.array_equal(R.bits(out), R.bits(flat)) and np.array_equal(rgb8, R.to_u8(flat))
        # ... also one with a -0 channel: where nothing is added the centre's bits come back, not -0 + 0 = +0
        flat[..., 1] = -0.0
        rgb8, out = twin_matches_reference(flat, pos, depth, cam, p)
        assert np.array_equal(R.bits(out), R.bits(flat)) and (R.bits(out[..., 1]) == 0x80000000).all()


def test_only_the_tiles_around_a_defocused_block_change():
    w, h, k = 96, 48, 16
    rad, _, _ = inputs(w, h)
    cam = camera(w, h)
    pos = np.zeros((h, w, 3), F)
    pos[..., 2] = -2.0
    pos[20:24, 40:44, 2] = -0.8  # tile (2, 1): l = 20 * |0.5 - 1.25| = 15
    depth = np.full((h, w), 2.0, F)
    rgb8, out = twin_matches_reference(rad, pos, depth, cam, lib.dof_params(max_radius=k, **DEFAULTS))
    changed = (R.bits(out) != R.bits(rad)).any(axis=-1)
    near = np.zeros((h, w), bool)
    near[0:48, 16:64] = True  # the 3 x 3 tiles around tile (2, 1)
    assert not changed[~near].any() and np.array_equal(rgb8[~near], R.to_u8(rad)[~near])
    outside = changed.copy()
    outside[20:24, 40:44] = False
    assert outside.any()  # the near block spreads over the sharp wall behind it


def test_a_sharp_foreground_keeps_its_edge_against_a_blurred_background():
    w, h = 64, 32
    cam = camera(w, h)
    pos = np.zeros((h, w, 3), F)
    pos[:, :w // 2, 2] = -2.0   # in focus, near
    pos[:, w // 2:, 2] = -6.0   # behind: l = 20 * |1/2 - 1/6| = 6.7
    rad = np.zeros((h, w, 3), F)
    rad[:, :w // 2] = 1.0
    rad[:, w // 2:] = 0.25
    rgb8, out = twin_matches_reference(rad, pos, np.full((h, w), 2.0, F), cam, lib.dof_params(**DEFAULTS))
    assert np.array_equal(R.bits(out[:, :w // 2]), R.bits(rad[:, :w // 2]))  # no background leaks into the foreground
    assert np.array_equal(R.bits(out), R.bits(rad))  # ... and a sharp foreground spreads nowhere: both sides are constant colours
    # the other way round: a defocused foreground (z = 0.8, l = 15) spreads over the sharp wall behind it
    pos[:, :w // 2, 2] = -0.8
    pos[:, w // 2:, 2] = -2.0
    rgb8, out = twin_matches_reference(rad, pos, np.full((h, w), 2.0, F), cam, lib.dof_params(**DEFAULTS))
    assert (out[:, w // 2:w // 2 + 8] > 0.25).any() and np.array_equal(R.bits(out[:, w // 2 + 17:]), R.bits(rad[:, w // 2 + 17:]))


def test_non_finite_pixels_spoil_only_themselves():
    w, h = 64, 64
    rad, pos, depth = inputs(w, h)
    cam = camera(w, h)
    spots = [(30, 30), (33, 27)]
    dirty, black = rad.copy(), rad.copy()
    dirty[spots[0]] = (np.nan, 0.5, 0.25)
    dirty[spots[1]] = np.inf
    mask = np.ones((h, w), bool)
    for s in spots:
        black[s] = 0.0
        mask[s] = False
    p = lib.dof_params(**DEFAULTS)
    rgb8, out = twin_matches_reference(dirty, pos, depth, cam, p)
    assert np.isfinite(out[mask]).all()
    for s in spots:
        assert np.array_equal(R.bits(out[s]), R.bits(dirty[s]))  # copied through
    want8, want = reference(black, pos, depth, cam, p, exclude=~mask)
    assert np.array_equal(R.bits(out[mask]), R.bits(want[mask])) and np.array_equal(rgb8[mask], want8[mask])
    clean = lib.depth_of_field_host(black, (pos, depth), cam, p)[1]
    assert (R.bits(clean[mask]) != R.bits(out[mask])).any()  # (the two pixels do lie under taps: leaving them out is seen)
    # non-finite position or depth is a miss; so are a depth <= 0 and a point at or behind the camera
    bad_pos, bad_depth, as_miss_pos, as_miss_depth = pos.copy(), depth.copy(), pos.copy(), depth.copy()
    hits = np.argwhere(depth > 0)
    for (y, x), v in zip(hits[:4], [(np.nan, 0.0, -1.0), (0.0, np.inf, -1.0), (0.0, 0.0, -np.inf), (0.0, 0.0, 1.0)]):
        bad_pos[y, x] = v
        as_miss_pos[y, x] = 0.0
        as_miss_depth[y, x] = 0.0
    for (y, x), z in zip(hits[4:8], [np.nan, np.inf, -np.inf, -2.0]):
        bad_depth[y, x] = z
        as_miss_depth[y, x] = 0.0
    assert_same(twin_matches_reference(rad, bad_pos, bad_depth, cam, p), lib.depth_of_field_host(rad, (as_miss_pos, as_miss_depth), cam, p))


@pytest.mark.parametrize("entry", ["ff_depth_of_field", "ff_depth_of_field_host"])
def test_invalid_arguments_are_refused_before_any_device_work(ff, entry):
    handle = ff.load()
    state = C.c_void_p(0x1)  # never dereferenced: every check below fails before the state is used
    w, h = 8, 4
    good_cam = camera(w, h)
    rad = np.zeros((h, w, 3), np.float32)
    pos = np.zeros((h, w, 3), np.float32)
    depth = np.zeros((h, w), np.float32)
    out = np.full((h, w, 3), 7.0, np.float32)
    rgb8 = np.full((h, w, 3), 7, np.uint8)
    ptr = lambda a: a.ctypes.data if a is not None else None  # noqa: E731

    def call(p, w=w, h=h, rad=rad, pos=pos, depth=depth, rgb8=rgb8, out=out, state=state, cam=good_cam):
        pp = C.byref(p) if p is not None else None
        cc = C.byref(cam) if cam is not None else None
        if entry == "ff_depth_of_field":
            return handle.ff_depth_of_field(state, cc, w, h, pp, ptr(rad), ptr(pos), ptr(depth), 0, ptr(rgb8), 0, ptr(out), 0)
        return handle.ff_depth_of_field_host(cc, w, h, pp, ptr(rad), ptr(pos), ptr(depth), ptr(rgb8), ptr(out))

    def refused(word, *args, **kw):
        assert call(*args, **kw) == T.FF_ERR_INVALID_ARG
        assert word in handle.ff_last_error().decode(), handle.ff_last_error()
    good = lib.dof_params(**DEFAULTS)
    nan, inf = float("nan"), float("inf")
    for field, values in [("focus_distance", (0.0, -1.0, nan, inf, 1e-45)), ("coc_scale", (-0.5, nan, inf)), ("max_radius", (0, 65, -3)),
                          ("grid", (0, 9, -1)), ("depth_extent", (0.0, -1.0, nan, inf)), ("flags", (1, -1)), ("reserved", ((1, 0), (0, 1)))]:
        for value in values:
            refused(field, lib.dof_params(**{field: value}))
    refused("params", None)
    refused("camera", good, cam=None)
    if entry == "ff_depth_of_field":
        refused("state", good, state=None)
    refused("radiance_in", good, rad=None)
    refused("position", good, pos=None)
    refused("depth", good, depth=None)
    for bw, bh in [(0, 4), (8, 0), (-1, 4), (8, 70000), (65536, 1)]:
        refused("size", good, bw, bh)
    for field in ("m_position", "m_forward"):
        for axis in "xyz":
            for value in (nan, inf):
                cam = camera(w, h)
                setattr(getattr(cam, field), axis, value)
                refused(field, good, cam=cam)
    # an output on top of an input, or overlapping it
    refused("radiance_out overlaps radiance_in", good, out=rad)
    big = np.zeros(h * w * 3 + 8, np.float32)
    refused("radiance_out overlaps radiance_in", good, rad=big[:h * w * 3].reshape(h, w, 3), out=big[8:].reshape(h, w, 3))
    refused("radiance_out overlaps position", good, out=big[:h * w * 3].reshape(h, w, 3), pos=big[8:].reshape(h, w, 3))
    refused("rgb8 overlaps depth", good, rgb8=depth.view(np.uint8))
    # the two outputs on each other
    both = np.zeros(h * w * 3 + 24, np.float32)  # (room for all of rgb8's h * w * 3 bytes from 4 floats before radiance_out's end)
    refused("rgb8 overlaps radiance_out", good, rgb8=both[h * w * 3 - 4:].view(np.uint8), out=both[:h * w * 3].reshape(h, w, 3))
    assert (out == 7.0).all() and (rgb8 == 7).all()
    # the edges of the ranges are accepted (host twin: it needs no state)
    if entry == "ff_depth_of_field_host":
        for edge in (dict(coc_scale=0.0), dict(max_radius=1, grid=1), dict(max_radius=64, grid=8), dict(focus_distance=1e-30)):
            assert call(lib.dof_params(**edge), rgb8=None) == T.FF_OK


def test_params_from_camera_checks_its_arguments(ff):
    handle = ff.load()
    cam = camera(64, 48)
    p = lib.dof_params(max_radius=9, grid=2, depth_extent=0.5)
    q = lib.dof_params_from_camera(cam, lib.camera_sampling(lens_radius=0.0, focus_distance=3.0), max_radius=9, grid=2, depth_extent=0.5)
    assert (q.focus_distance, q.coc_scale, q.max_radius, q.grid, q.depth_extent) == (3.0, 0.0, 9, 2, F(0.5))
    good = lib.camera_sampling(lens_radius=0.08, focus_distance=2.5)
    for args, word in [((None, C.byref(good), C.byref(p)), "camera"), ((C.byref(cam), None, C.byref(p)), "sampling"), ((C.byref(cam), C.byref(good), None), "params")]:
        assert handle.ff_dof_params_from_camera(*args) == T.FF_ERR_INVALID_ARG and word in handle.ff_last_error().decode()
    for bad, word in [(dict(lens_radius=-1.0), "lens_radius"), (dict(lens_radius=float("nan")), "lens_radius"), (dict(lens_radius=0.1, focus_distance=0.0), "focus_distance"),
                      (dict(focus_distance=float("inf")), "focus_distance"), (dict(pixel_filter=7), "pixel_filter")]:
        cs = lib.camera_sampling(**bad)
        assert handle.ff_dof_params_from_camera(C.byref(cam), C.byref(cs), C.byref(p)) == T.FF_ERR_INVALID_ARG
        assert word in handle.ff_last_error().decode()
    cs = lib.camera_sampling(lens_radius=0.08, focus_distance=2.5)
    cs.reserved = 1
    assert handle.ff_dof_params_from_camera(C.byref(cam), C.byref(cs), C.byref(p)) == T.FF_ERR_INVALID_ARG
    assert (p.focus_distance, p.coc_scale, p.max_radius) == (1.0, 0.0, 9)  # nothing was written


def pinhole_pixel(cam, points):
    """World points -> pixel coordinates (x right, y down) of the pinhole camera, in float64: m_fov is the vertical field of
    view and pixels are square."""
    e = points.astype(np.float64) - vec(cam.m_position).astype(np.float64)
    z = e @ vec(cam.m_forward).astype(np.float64)
    s = 0.5 * cam.m_screenHeight / math.tan(math.radians(cam.m_fov) / 2)
    x = (e @ vec(cam.m_right).astype(np.float64)) / z * s + 0.5 * cam.m_screenWidth
    y = -(e @ vec(cam.m_up).astype(np.float64)) / z * s + 0.5 * cam.m_screenHeight
    return np.stack([x, y], axis=-1)


@pytest.mark.parametrize("fov", [None, 38.0], ids=["default_fov", "fov38"])
def test_the_scale_is_the_thin_lens_circle_of_confusion(fov):
    """ff_dof_params_from_camera against the rays of the in-path thin lens (ff_camera_sample_rays): the rays of 4096 samples of a
    pixel, cut by the plane at axial depth z and projected through the pinhole, lie in a disk of coc_scale |1/focus - 1/z| pixels
    around the pixel's own pinhole point.  The largest of 4096 uniform-area lens radii exceeds 0.97 R (it falls short with
    probability (0.97^2)^4096 < 1e-100); the upper bound is float rounding."""
    w, h, samples = 64, 48, 4096
    cam = scenes.posed_camera(w, h, position=(0.3, -0.2, 2.4), yaw=-70.0, pitch=12.0)
    if fov is not None:
        cam.m_fov = fov
    focus = 2.5
    cs = lib.camera_sampling(T.PIXEL_CORNER, lens_radius=0.08, focus_distance=focus)
    p = lib.dof_params_from_camera(cam, cs)
    assert p.focus_distance == F(focus)
    want = float(cs.lens_radius) * 0.5 * h / math.tan(math.radians(float(cam.m_fov)) / 2)  # (python floats: double)
    assert p.coc_scale == F(want)  # (evaluated in double, rounded once)
    origin, fwd = vec(cam.m_position).astype(np.float64), vec(cam.m_forward).astype(np.float64)
    for x, y in [(w // 2, h // 2), (0, 0), (w - 1, h - 1), (w - 1, 0)]:
        n = np.arange(samples)
        o, d = lib.camera_sample_rays(cam, cs, w, 99, np.full(samples, x), np.full(samples, y), n)
        o0, d0 = lib.camera_sample_rays(cam, lib.camera_sampling(), w, 99, [x], [y], [0])
        o, d, o0, d0 = (a.astype(np.float64) for a in (o, d, o0, d0))
        for z in (1.0, 1.5, 4.0, 10.0):
            at = lambda oo, dd: oo + dd * ((z - (oo - origin) @ fwd) / (dd @ fwd))[:, None]  # noqa: E731
            centre = pinhole_pixel(cam, at(o0, d0))[0]
            spread = np.linalg.norm(pinhole_pixel(cam, at(o, d)) - centre, axis=-1).max()
            radius = float(p.coc_scale) * abs(1.0 / focus - 1.0 / z)
            print(f"pixel ({x}, {y}) z {z}: largest distance {spread:.6f} px, coc_scale |1/focus - 1/z| = {radius:.6f}, ratio {spread / radius:.6f}")
            assert 0.97 * radius <= spread <= 1.001 * radius
