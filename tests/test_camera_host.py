"""Per-sample camera rays on the host (ff_camera_sample_rays, no GPU): the twin against the float32 restatement of the estimator
(tests/camera_ref.py) bit for bit, the defaults against primary_ray's formula, the geometry and the statistics of the lens and the
box filter in float64, the scene file's keys, and the argument checks."""
import ctypes as C

import numpy as np
import pytest

from gpupathtracer_amd import lib, scenes
from gpupathtracer_amd import types as T
import camera_ref

SEEDS = (7, (5 << 32) | 99)  # (the second is above 2^32: the frame key folds its high word in)


def cameras():
    return {
        "default": scenes.default_camera(64, 48),
        "posed": scenes.posed_camera(64, 48, position=(0.3, 0.2, 2.4), yaw=-70.0, pitch=12.0),
        "non_square": scenes.posed_camera(57, 31, position=(0.0, 0.5, 3.0), yaw=-95.0, pitch=-6.0),
    }


def settings():
    return {
        "box": lib.camera_sampling(T.PIXEL_BOX),
        "lens": lib.camera_sampling(T.PIXEL_CORNER, 0.3, 4.0),
        "both": lib.camera_sampling(T.PIXEL_BOX, 0.05, 2.5),
    }


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def size(cam):
    return int(cam.m_screenWidth), int(cam.m_screenHeight)


def samples_of(cam, n, rng):
    w, h = size(cam)
    return rng.integers(0, w, n), rng.integers(0, h, n), rng.integers(0, 1500, n)


# ---- 1. the twin is the estimator, bit for bit --------------------------------------------------------------------------------------

@pytest.mark.parametrize("cam_name", ["default", "posed", "non_square"])
@pytest.mark.parametrize("setting", ["box", "lens", "both"])
@pytest.mark.parametrize("seed", SEEDS)
def test_twin_equals_the_reference_bit_for_bit(cam_name, setting, seed):
    cam, cs = cameras()[cam_name], settings()[setting]
    xs, ys, ss = samples_of(cam, 3000, np.random.default_rng(11))
    w = size(cam)[0]
    # (a jitter is passed on purpose: BOX frames must ignore it, CORNER frames apply it)
    o, d = lib.camera_sample_rays(cam, cs, w, seed, xs, ys, ss, jitter=(0.25, 0.5))
    ro, rd = camera_ref.sample_rays(cam, cs, w, seed, xs, ys, ss, jitter=(0.25, 0.5))
    assert np.array_equal(bits(o), bits(ro))
    assert np.array_equal(bits(d), bits(rd))
    if cs.pixel_filter == T.PIXEL_BOX:
        o0, d0 = lib.camera_sample_rays(cam, cs, w, seed, xs, ys, ss)
        assert np.array_equal(bits(o), bits(o0)) and np.array_equal(bits(d), bits(d0))
    # the streams are the sample's own: another seed, another ray
    o1, d1 = lib.camera_sample_rays(cam, cs, w, seed + 1, xs, ys, ss, jitter=(0.25, 0.5))
    assert not np.array_equal(bits(d), bits(d1))


# ---- 2. the defaults are primary_ray --------------------------------------------------------------------------------------------------

def primary_ray_formula(cam, jitter, xs, ys):
    """kernel.cu:197-205 as ff_k_shade.h's primary_ray evaluates it, on the jittered matrix."""
    m = camera_ref.ray_matrix(cam, jitter)
    f = np.float32
    px = (xs.astype(np.float32) / f(cam.m_screenWidth)) * f(2) - f(1)
    py = f(1) - (ys.astype(np.float32) / f(cam.m_screenHeight)) * f(2)
    far = f(cam.m_farClip)
    v0, v1, v2, v3 = px * far, py * far, f(1) * far, f(1) * far
    w = np.stack([(m[0, k] * v0 + m[1, k] * v1) + (m[2, k] * v2 + m[3, k] * v3) for k in range(3)], -1)
    dd = w - camera_ref.vec(cam.m_position)
    inv = f(1) / np.sqrt((dd[:, 0] * dd[:, 0] + dd[:, 1] * dd[:, 1]) + dd[:, 2] * dd[:, 2])
    return dd * inv[:, None]


@pytest.mark.parametrize("cam_name", ["default", "posed", "non_square"])
@pytest.mark.parametrize("jitter", [(0.0, 0.0), (0.375, 0.8125)])
def test_defaults_are_the_primary_ray(cam_name, jitter):
    cam = cameras()[cam_name]
    xs, ys, ss = samples_of(cam, 2000, np.random.default_rng(3))
    want = primary_ray_formula(cam, jitter, xs, ys)
    pos = camera_ref.vec(cam.m_position)
    for cs in (None, lib.camera_sampling()):
        o, d = lib.camera_sample_rays(cam, cs, size(cam)[0], 99, xs, ys, ss, jitter=jitter)
        assert np.array_equal(bits(d), bits(want))
        assert np.array_equal(bits(o), bits(np.broadcast_to(pos, o.shape)))
    # every sample of a pixel is the same ray
    o2, d2 = lib.camera_sample_rays(cam, None, size(cam)[0], 99, xs, ys, ss + 17, jitter=jitter)
    assert np.array_equal(bits(d2), bits(want))


# ---- 3. geometry and statistics, in float64 from the twin's output ----------------------------------------------------------------

@pytest.mark.parametrize("cam_name", ["default", "posed", "non_square"])
def test_lens_rays_pass_the_focus_point_and_start_on_the_lens(cam_name):
    cam = cameras()[cam_name]
    radius, focus = 0.3, 4.0
    cs = lib.camera_sampling(T.PIXEL_CORNER, radius, focus)
    xs, ys, ss = samples_of(cam, 4000, np.random.default_rng(5))
    w = size(cam)[0]
    o, d = (a.astype(np.float64) for a in lib.camera_sample_rays(cam, cs, w, 31, xs, ys, ss))
    po, pd = (a.astype(np.float64) for a in lib.camera_sample_rays(cam, None, w, 31, xs, ys, ss))
    fwd, right, up, pos = (camera_ref.vec(v).astype(np.float64) for v in (cam.m_forward, cam.m_right, cam.m_up, cam.m_position))
    point = po + pd * (focus / (pd @ fwd))[:, None]  # the pinhole ray's point in the plane of focus
    # distance of the point from the sample's ray
    rel = point - o
    off = rel - d * np.sum(rel * d, -1)[:, None]
    assert np.linalg.norm(off, axis=-1).max() <= 1e-5 * focus
    # origins: in the lens plane, within the radius
    lo = o - pos
    assert np.abs(lo @ fwd).max() <= 1e-6
    r = np.hypot(lo @ right, lo @ up)
    assert r.max() <= radius * (1 + 1e-6) and r.max() > 0.9 * radius


def test_lens_points_are_uniform_on_the_disc():
    cam = cameras()["posed"]
    radius, n = 0.3, 4096
    cs = lib.camera_sampling(T.PIXEL_CORNER, radius, 4.0)
    o, _ = lib.camera_sample_rays(cam, cs, 64, 2024, np.full(n, 17), np.full(n, 9), np.arange(n))
    right, up, pos = (camera_ref.vec(v).astype(np.float64) for v in (cam.m_right, cam.m_up, cam.m_position))
    lo = o.astype(np.float64) - pos
    a, b = lo @ right, lo @ up
    # a uniform disc of radius R: each coordinate has variance R^2 / 4; r^2 has mean R^2 / 2 and variance R^4 / 12
    se = radius / 2 / np.sqrt(n)
    assert abs(a.mean()) <= 5 * se and abs(b.mean()) <= 5 * se
    r2 = a * a + b * b
    assert abs(r2.mean() - radius ** 2 / 2) <= 5 * (radius ** 2 / np.sqrt(12.0)) / np.sqrt(n)


def test_box_offsets_are_uniform_in_the_pixel():
    cam = cameras()["default"]  # (its right and up are the image's axes)
    n, x, y = 4096, 40, 13
    w, h = size(cam)
    cs = lib.camera_sampling(T.PIXEL_BOX)
    _, d = lib.camera_sample_rays(cam, cs, w, 5, np.full(n, x), np.full(n, y), np.arange(n))
    # recover Px, Py from the direction: the pixel grid is affine in the image plane, spanned by three corner rays
    xs, ys = np.array([x, x + 1, x]), np.array([y, y, y + 1])
    _, corner = lib.camera_sample_rays(cam, None, w, 5, xs, ys, np.zeros(3, int))
    fwd = camera_ref.vec(cam.m_forward).astype(np.float64)
    plane = lambda v: v.astype(np.float64) / (v.astype(np.float64) @ fwd)[:, None]  # noqa: E731
    q, c = plane(d), plane(corner)
    ex, ey = c[1] - c[0], c[2] - c[0]
    fx = (q - c[0]) @ ex / (ex @ ex)
    fy = (q - c[0]) @ ey / (ey @ ey)
    tol = 1e-4  # (float32 directions: the recovered offset is good to about 1e-5 of a pixel)
    assert fx.min() >= -tol and fx.max() < 1 + tol and fy.min() >= -tol and fy.max() < 1 + tol
    se = np.sqrt(1.0 / 12.0 / n)
    assert abs(fx.mean() - 0.5) <= 5 * se and abs(fy.mean() - 0.5) <= 5 * se
    # ... and they are the documented stream's numbers, which lie in [0, 1) exactly (the twin is the reference bit for bit: test 1)
    rx, ry = camera_ref.pixel_offsets(cs, w, 5, np.full(n, x), np.full(n, y), np.arange(n))
    assert rx.min() >= 0.0 and rx.max() < 1.0 and ry.min() >= 0.0 and ry.max() < 1.0
    assert abs(rx.astype(np.float64).mean() - 0.5) <= 5 * se and abs(ry.astype(np.float64).mean() - 0.5) <= 5 * se
    assert np.abs(fx - rx).max() <= tol and np.abs(fy - ry).max() <= tol


# ---- 4. the scene file ------------------------------------------------------------------------------------------------------------------

def write_scene(tmp_path, text):
    path = str(tmp_path / "scene.ff")
    with open(path, "w") as f:
        f.write(text)
    return path


BODY = "bxdf grey diffuse albedo 0.5 0.5 0.5\nplane position 0 0 -2 bxdf grey\n"


def test_scene_file_camera_keys(tmp_path):
    sf = lib.SceneFile(write_scene(tmp_path, "# a lens\ncamera position 0 0 3 aperture 0.25 focus 3.5 filter box fov 60\n" + BODY))
    try:
        cs = sf.camera_sampling()
        assert (cs.pixel_filter, cs.lens_radius, cs.focus_distance, cs.reserved) == (T.PIXEL_BOX, 0.25, 3.5, 0)
        cam = sf.camera(32, 24)
        assert (cam.m_position.z, cam.m_fov) == (3.0, 60.0)  # (the other keys go on being read around the new ones)
    finally:
        sf.close()
    sf = lib.SceneFile(write_scene(tmp_path, "camera aperture 0.5\n" + BODY))
    try:
        cs = sf.camera_sampling()
        assert (cs.pixel_filter, cs.lens_radius, cs.focus_distance) == (T.PIXEL_CORNER, 0.5, 1.0)  # (keys not given keep the defaults)
    finally:
        sf.close()
    # a focus <= 0 is a setting ff_set_camera_sampling takes while there is no lens: so does the file
    sf = lib.SceneFile(write_scene(tmp_path, "camera focus -1 filter box\n" + BODY))
    try:
        cs = sf.camera_sampling()
        assert (cs.pixel_filter, cs.lens_radius, cs.focus_distance) == (T.PIXEL_BOX, 0.0, -1.0)
    finally:
        sf.close()
    sf = lib.SceneFile(write_scene(tmp_path, "camera filter corner\n" + BODY))
    try:
        assert sf.camera_sampling().pixel_filter == T.PIXEL_CORNER
    finally:
        sf.close()


@pytest.mark.parametrize("text", ["camera position 0 0 3 fov 60\n" + BODY, BODY])
def test_scene_file_without_the_keys(tmp_path, text):
    sf = lib.SceneFile(write_scene(tmp_path, text))
    try:
        assert sf.camera_sampling() is None
        out = lib.camera_sampling(T.PIXEL_BOX, 0.7, 9.0)
        assert lib.load().ff_scene_file_camera_sampling(sf._handle, C.byref(out)) == 0
        assert (out.pixel_filter, out.lens_radius, out.focus_distance) == (T.PIXEL_BOX, np.float32(0.7), 9.0)  # (left alone)
    finally:
        sf.close()


@pytest.mark.parametrize("text,line", [
    ("camera aperture -0.1\n" + BODY, 1),
    (BODY + "camera aperture 0.2 focus 0\n", 3),
    ("camera focus -1 aperture 0.2\n" + BODY, 1),
    ("\ncamera filter tent\n" + BODY, 2),
    ("camera position 0 0 3 aperture lots\n" + BODY, 1),
])
def test_scene_file_camera_key_errors(tmp_path, text, line):
    path = write_scene(tmp_path, text)
    with pytest.raises(lib.FireflyError) as e:
        lib.SceneFile(path)
    assert e.value.status == T.FF_ERR_INVALID_ARG
    assert f"{path}:{line}:" in e.value.message


# ---- 5. argument checks -------------------------------------------------------------------------------------------------------------------

def last_error():
    return lib.load().ff_last_error().decode("utf-8", "replace")


def call(cam, cs, width, xs, ys, ss, n, o, d, jitter=(0.0, 0.0)):
    ptr = lambda a: None if a is None else a.ctypes.data  # noqa: E731
    return lib.load().ff_camera_sample_rays(None if cam is None else C.byref(cam), None if cs is None else C.byref(cs), jitter[0], jitter[1], width, 1,
                                            ptr(xs), ptr(ys), ptr(ss), n, ptr(o), ptr(d))


def test_argument_checks():
    cam = cameras()["default"]
    xs, ys, ss = (np.array([1, 2], np.int32) for _ in range(3))
    o, d = np.zeros((2, 3), np.float32), np.zeros((2, 3), np.float32)
    assert call(cam, None, 64, xs, ys, ss, 2, o, d) == T.FF_OK
    assert call(cam, None, 64, None, None, None, 0, None, None) == T.FF_OK
    assert call(None, None, 64, xs, ys, ss, 2, o, d) == T.FF_ERR_INVALID_ARG
    for k in range(5):
        args = [xs, ys, ss, o, d]
        args[k] = None
        assert call(cam, None, 64, args[0], args[1], args[2], 2, args[3], args[4]) == T.FF_ERR_INVALID_ARG, k
    assert call(cam, None, 64, xs, ys, ss, -1, o, d) == T.FF_ERR_INVALID_ARG
    assert "n must not be negative" in last_error()
    assert call(cam, None, 0, xs, ys, ss, 2, o, d) == T.FF_ERR_INVALID_ARG
    assert call(cam, None, 64, xs, ys, ss, 2, o, d, jitter=(1.0, 0.0)) == T.FF_ERR_INVALID_ARG
    assert call(cam, None, 64, np.array([1, -2], np.int32), ys, ss, 2, o, d) == T.FF_ERR_INVALID_ARG
    assert call(cam, None, 64, xs, ys, np.array([-1, 0], np.int32), 2, o, d) == T.FF_ERR_INVALID_ARG


def bad_settings():
    def make(**kw):
        cs = lib.camera_sampling()
        for k, v in kw.items():
            setattr(cs, k, v)
        return cs
    return [
        (make(pixel_filter=2), "pixel_filter"), (make(pixel_filter=-1), "pixel_filter"),
        (make(lens_radius=-0.5), "lens_radius"), (make(lens_radius=float("nan")), "lens_radius"), (make(lens_radius=float("inf")), "lens_radius"),
        (make(focus_distance=float("nan")), "focus_distance"), (make(focus_distance=float("inf")), "focus_distance"),
        (make(lens_radius=0.1, focus_distance=0.0), "focus_distance"), (make(lens_radius=0.1, focus_distance=-2.0), "focus_distance"),
        (make(reserved=3), "reserved"),
    ]


def test_invalid_settings_name_the_field():
    cam = cameras()["default"]
    xs, ys, ss = (np.array([1, 2], np.int32) for _ in range(3))
    o, d = np.zeros((2, 3), np.float32), np.zeros((2, 3), np.float32)
    for cs, field in bad_settings():
        assert call(cam, cs, 64, xs, ys, ss, 2, o, d) == T.FF_ERR_INVALID_ARG, field
        assert field in last_error()
    # a focus <= 0 is fine while there is no lens
    ok = lib.camera_sampling(T.PIXEL_BOX, 0.0, -1.0)
    assert call(cam, ok, 64, xs, ys, ss, 2, o, d) == T.FF_OK


def test_init_gives_todays_camera():
    cs = T.FfCameraSampling(9, 9.0, 9.0, 9)
    lib.load().ff_camera_sampling_init(C.byref(cs))
    assert (cs.pixel_filter, cs.lens_radius, cs.focus_distance, cs.reserved) == (T.PIXEL_CORNER, 0.0, 1.0, 0)
    lib.load().ff_camera_sampling_init(None)
