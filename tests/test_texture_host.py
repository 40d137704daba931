"""Albedo textures without a GPU: the host twins of the kernels' lookup (ff_texture_sample, ff_surface_uv) against the float32
restatement of tests/texture_ref.py and float64, the argument checks that need no device, the PPM reader and the byte-to-linear
table, and the scene file's texture / albedo_map statements."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from gpupathtracer_amd import lib, scenes
from gpupathtracer_amd import types as T
import texture_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["ff_texture_create", "ff_texture_destroy", "ff_set_albedo_texture", "ff_texture_sample", "ff_surface_uv", "ff_load_ppm", "ff_free_ppm",
       "ff_rgb8_to_linear", "ff_scene_file_texture_count", "ff_scene_file_texture", "ff_scene_file_albedo_map"]
ALL_FLAGS = [T.TEX_REPEAT | T.TEX_BILINEAR, T.TEX_CLAMP | T.TEX_BILINEAR, T.TEX_REPEAT | T.TEX_NEAREST, T.TEX_CLAMP | T.TEX_NEAREST]
SIZES = [(1, 1), (1, 7), (7, 1), (5, 3), (13, 11), (16, 8), (100, 37)]  # (W, H)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def texture(w, h, seed=0):
    return np.random.default_rng(seed).random((h, w, 3)).astype(np.float32)


def coordinates(w, h, seed=1):
    """Random coordinates in and far outside [0, 1], every texel centre, every texel edge and corner."""
    rng = np.random.default_rng(seed)
    parts = [rng.random((400, 2)), rng.uniform(-3.0, 4.0, (400, 2)), rng.uniform(-1.0e4, 1.0e4, (200, 2)), rng.uniform(-1.0e9, 1.0e9, (50, 2)),
             rng.uniform(-1.0e30, 1.0e30, (20, 2))]
    cx, cy = (np.arange(w) + 0.5) / w, (np.arange(h) + 0.5) / h
    ex, ey = np.arange(-w, 2 * w + 1) / w, np.arange(-h, 2 * h + 1) / h
    parts.append(np.stack(np.meshgrid(cx, cy), -1).reshape(-1, 2))
    parts.append(np.stack(np.meshgrid(ex, ey), -1).reshape(-1, 2))
    parts.append(np.stack(np.meshgrid(cx, ey), -1).reshape(-1, 2))
    return np.concatenate(parts).astype(np.float32)


def test_new_names_are_exported_and_declared(ff):
    handle = ff.load()
    header = open(os.path.join(ROOT, "include", "firefly", "ff_api.h")).read()
    declared = set(re.findall(r"FF_API\s+[\w\s\*]+?\b(ff_\w+)\s*\(", header))
    for name in NEW:
        assert name in ff.EXPORTS and name in declared and hasattr(handle, name), name
    types_h = open(os.path.join(ROOT, "include", "firefly", "ff_types.h")).read()
    for name, value in [("FF_TEX_REPEAT", T.TEX_REPEAT), ("FF_TEX_CLAMP", T.TEX_CLAMP), ("FF_TEX_BILINEAR", T.TEX_BILINEAR), ("FF_TEX_NEAREST", T.TEX_NEAREST)]:
        assert re.search(r"#define\s+%s\s+%d\b" % (name, value), types_h), name


# ---- the texel lookup ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("flags", ALL_FLAGS)
@pytest.mark.parametrize("size", SIZES)
def test_sample_equals_the_float32_restatement(size, flags):
    w, h = size
    rgb = texture(w, h, seed=w * 100 + h)
    uv = coordinates(w, h)
    got = lib.texture_sample(rgb, uv, flags)
    ref = texture_ref.sample(rgb, uv, flags)
    assert np.array_equal(bits(got), bits(ref)), np.argwhere(bits(got) != bits(ref))[:5]


@pytest.mark.parametrize("flags", ALL_FLAGS)
def test_texel_centres_return_the_texel(flags):
    w, h = 8, 4  # (powers of two: the centres' coordinates and s, t are exact)
    rgb = texture(w, h, seed=3)
    x, y = np.meshgrid(np.arange(w), np.arange(h))
    uv = np.stack([(x + 0.5) / w, 1.0 - (y + 0.5) / h], -1).astype(np.float32)
    assert np.array_equal(bits(lib.texture_sample(rgb, uv, flags)), bits(rgb))


@pytest.mark.parametrize("flags", ALL_FLAGS)
@pytest.mark.parametrize("size", [(1, 1), (5, 3), (16, 8)])
def test_constant_texture_and_non_finite_coordinates(size, flags):
    w, h = size
    value = np.array([0.3, 0.7123, 1.0e-3], np.float32)
    const = np.broadcast_to(value, (h, w, 3)).copy()
    special = np.array([np.nan, np.inf, -np.inf, 3.4e38, -3.4e38, 1e-45, -1e-45, 0.0, -0.0, 1.0, -1.0], np.float32)
    uv = np.concatenate([coordinates(w, h), np.stack(np.meshgrid(special, special), -1).reshape(-1, 2)])
    got = lib.texture_sample(const, uv, flags)
    assert np.array_equal(bits(got), bits(np.broadcast_to(value, got.shape)))
    # a non-finite coordinate reads as 0 (ff_api.h): an in-range texel, the one (0, v) or (u, 0) gives
    rgb = texture(w, h, seed=9)
    for bad in (np.nan, np.inf, -np.inf):
        for other in (0.25, 0.9, -7.5):
            a = lib.texture_sample(rgb, np.array([[bad, other], [other, bad], [bad, bad]], np.float32), flags)
            b = lib.texture_sample(rgb, np.array([[0.0, other], [other, 0.0], [0.0, 0.0]], np.float32), flags)
            assert np.array_equal(bits(a), bits(b))
    # every bit pattern class stays inside the texture's range of values
    pats = np.random.default_rng(4).integers(0, 2 ** 32, (4000, 2), dtype=np.uint64).astype(np.uint32).view(np.float32)
    out = lib.texture_sample(rgb, pats, flags)
    assert np.all(np.isfinite(out)) and out.min() >= rgb.min() and out.max() <= rgb.max()


@pytest.mark.parametrize("flags", [T.TEX_REPEAT | T.TEX_BILINEAR, T.TEX_REPEAT | T.TEX_NEAREST])
@pytest.mark.parametrize("size", [(5, 3), (16, 8), (100, 37)])
def test_repeat_is_periodic(size, flags):
    w, h = size
    rgb = texture(w, h, seed=11)
    rng = np.random.default_rng(12)
    base = (rng.integers(0, 1 << 12, (2000, 2)) / float(1 << 12)).astype(np.float32)  # 12 fraction bits: uv + k is exact for |k| < 2^11
    ref = lib.texture_sample(rgb, base, flags)
    for k in (1, -1, 2, -5, 17, 1000, -2047):
        moved = (base + np.float32(k)).astype(np.float32)
        assert np.array_equal(moved.astype(np.float64), base.astype(np.float64) + k)  # (exactly representable)
        assert np.array_equal(bits(lib.texture_sample(rgb, moved, flags)), bits(ref)), k
        mixed = base.copy()
        mixed[:, 0] += np.float32(k)
        assert np.array_equal(bits(lib.texture_sample(rgb, mixed, flags)), bits(ref)), k


def test_clamp_holds_the_border_texels():
    w, h = 6, 4
    rgb = texture(w, h, seed=13)
    far = np.array([[-3.0, 0.5 / h], [9.0, 1.0 - 0.5 / h], [-1e20, -1e20], [1e20, 1e20]], np.float32)
    for flags in (T.TEX_CLAMP, T.TEX_CLAMP | T.TEX_NEAREST):
        got = lib.texture_sample(rgb, far, flags)
        assert np.array_equal(bits(got), bits(np.stack([rgb[h - 1, 0], rgb[0, w - 1], rgb[h - 1, 0], rgb[0, w - 1]])))


def test_sample_argument_checks():
    rgb = texture(4, 4)
    uv = np.zeros((1, 2), np.float32)
    for bad in (-1.0, np.nan, np.inf):
        t = rgb.copy()
        t[1, 2, 0] = bad
        with pytest.raises(lib.FireflyError) as e:
            lib.texture_sample(t, uv)
        assert e.value.status == T.FF_ERR_INVALID_ARG
    for flags in (4, 8, -1, 256):
        with pytest.raises(lib.FireflyError) as e:
            lib.texture_sample(rgb, uv, flags)
        assert e.value.status == T.FF_ERR_INVALID_ARG
    handle = lib.load()
    out = np.zeros(3, np.float32)
    for w, h in ((0, 4), (4, 0), (-1, 4), (1 << 14, (1 << 12) + 1)):
        assert handle.ff_texture_sample(rgb.ctypes.data, w, h, 0, uv.ctypes.data, 1, out.ctypes.data) == T.FF_ERR_INVALID_ARG
    assert handle.ff_texture_sample(None, 4, 4, 0, uv.ctypes.data, 1, out.ctypes.data) == T.FF_ERR_INVALID_ARG


def test_state_calls_reject_null_arguments_without_a_device():
    handle = lib.load()
    rgb = texture(2, 2)
    tid = C.c_int(7)
    assert handle.ff_texture_create(None, rgb.ctypes.data, 2, 2, 0, C.byref(tid)) == T.FF_ERR_INVALID_ARG
    assert handle.ff_texture_destroy(None, 0) == T.FF_ERR_INVALID_ARG
    assert handle.ff_set_albedo_texture(None, 0, 0, 1.0, 1.0, 0.0, 0.0) == T.FF_ERR_INVALID_ARG


# ---- the surface coordinate -----------------------------------------------------------------------------------------------------

def world_of(scene, gi, object_points):
    m = np.array(list(scene.geometries[gi].m_modelMatrix.m), np.float64).reshape(4, 4).T
    return np.asarray(object_points, np.float64) @ m[:3, :3].T + m[:3, 3]


def test_surface_uv_of_fixture_triangles():
    wahoo = scenes.load_mesh("wahoo")
    scene = scenes.open_floor_scene(area_light=True, wahoo=wahoo)
    assert np.abs(wahoo[:, 9:15]).max() > 0.0  # (the fixture carries UVs)
    idx = np.arange(0, len(wahoo), 7)
    t = wahoo[idx].astype(np.float64)
    v0, v1, v2 = t[:, 0:3], t[:, 3:6], t[:, 6:9]
    uv0, uv1, uv2 = t[:, 9:11], t[:, 11:13], t[:, 13:15]
    span = np.abs(np.stack([uv0, uv1, uv2])).max() + 1.0
    for wts in ((1 / 3, 1 / 3, 1 / 3), (0.5, 0.5, 0.0), (0.0, 0.5, 0.5), (0.5, 0.0, 0.5)):
        obj = wts[0] * v0 + wts[1] * v1 + wts[2] * v2
        expect = wts[0] * uv0 + wts[1] * uv1 + wts[2] * uv2
        world = world_of(scene, 0, obj)
        got = lib.surface_uv(scene, 0, world, idx).astype(np.float64)
        ref = texture_ref.surface_uv64(scene, 0, world.astype(np.float32), wahoo, idx)
        # float32 barycentrics of a point rounded to float32: a few 1e-6 for well-shaped triangles; slivers (small den) lose more,
        # so the bound scales with the conditioning den / (|e1|^2 |e2|^2) of each triangle
        e1, e2 = v1 - v0, v2 - v0
        cond = (np.sum(e1 * e1, 1) * np.sum(e2 * e2, 1)) / np.maximum(np.sum(e1 * e1, 1) * np.sum(e2 * e2, 1) - np.sum(e1 * e2, 1) ** 2, 1e-300)
        tol = 2e-5 * span * cond
        assert np.all(np.abs(got - ref).max(1) <= tol), np.abs(got - ref).max()
        assert np.all(np.abs(got - expect).max(1) <= 4 * tol + 1e-4 * span)


def test_surface_uv_of_planes_and_spheres():
    s = scenes.Scene()
    s.add_plane((0.5, -1.0, 2.0), (90, 0, 0), (4, 2, 1), scenes.make_bxdf(T.BXDF_DIFFUSE, albedo=(1, 1, 1)))
    s.add_plane((0, 0, 0), (0, 0, 0), (1, 1, 1), scenes.make_bxdf(T.BXDF_DIFFUSE, albedo=(1, 1, 1)))
    s.add_sphere(2.0, (1.0, 2.0, 3.0), (0, 0, 0), (1, 1, 1), scenes.make_bxdf(T.BXDF_DIFFUSE, albedo=(1, 1, 1)))
    scene = s.finalize()
    corners = np.array([[-0.5, -0.5, 0], [0.5, -0.5, 0], [-0.5, 0.5, 0], [0.5, 0.5, 0], [0, 0, 0]], np.float64)
    expect = np.array([[0, 0], [1, 0], [0, 1], [1, 1], [0.5, 0.5]], np.float64)
    assert np.array_equal(lib.surface_uv(scene, 1, corners).astype(np.float64), expect)  # (identity transform: exact)
    got = lib.surface_uv(scene, 0, world_of(scene, 0, corners)).astype(np.float64)
    assert np.abs(got - expect).max() <= 1e-6
    # sphere: +Y is v = 1, -Y is v = 0, -Z is u = 0, +X is u = 1/4
    centre = np.array([1.0, 2.0, 3.0])
    dirs = np.array([[0, 1, 0], [0, -1, 0], [0, 0, -1], [1, 0, 0], [0, 0, 1], [-1, 0, 0]], np.float64)
    got = lib.surface_uv(scene, 2, centre + 2.0 * dirs).astype(np.float64)
    assert abs(got[0, 1] - 1.0) <= 1e-6 and abs(got[1, 1]) <= 1e-6
    assert np.abs(got[2:, 1] - 0.5).max() <= 1e-6
    assert np.abs(got[2:, 0] - np.array([0.0, 0.25, 0.5, 0.75])).max() <= 1e-6
    rng = np.random.default_rng(2)
    d = rng.normal(size=(500, 3))
    pts = (centre + 2.0 * d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    got = lib.surface_uv(scene, 2, pts).astype(np.float64)
    ref = texture_ref.surface_uv64(scene, 2, pts)
    du = np.abs(got[:, 0] - ref[:, 0])
    assert np.minimum(du, 1.0 - du).max() <= 1e-5 and np.abs(got[:, 1] - ref[:, 1]).max() <= 1e-5
    assert np.all((got[:, 0] >= 0.0) & (got[:, 0] <= 1.0))


def test_surface_uv_argument_checks():
    scene = scenes.open_floor_scene(area_light=False)
    p = np.zeros((1, 3), np.float32)
    for gi in (-1, 2, 99):
        with pytest.raises(lib.FireflyError) as e:
            lib.surface_uv(scene, gi, p)
        assert e.value.status == T.FF_ERR_INVALID_ARG
    with pytest.raises(lib.FireflyError) as e:
        lib.surface_uv(scene, 0, p)  # a mesh needs triangle indices
    assert e.value.status == T.FF_ERR_INVALID_ARG
    for ti in (-1, 10 ** 7):
        with pytest.raises(lib.FireflyError) as e:
            lib.surface_uv(scene, 0, p, [ti])
        assert e.value.status == T.FF_ERR_INVALID_ARG


# ---- image files --------------------------------------------------------------------------------------------------------------

def test_ppm_round_trips(tmp_path):
    rng = np.random.default_rng(6)
    img = rng.integers(0, 256, (7, 5, 3)).astype(np.uint8)
    p3 = str(tmp_path / "a.ppm")
    lib.save_ppm(p3, img)
    back = lib.load_ppm(p3)
    assert back.dtype == np.uint8 and np.array_equal(back, img)
    again = str(tmp_path / "b.ppm")
    lib.save_ppm(again, back)
    assert open(p3, "rb").read() == open(again, "rb").read()
    p6 = str(tmp_path / "c.ppm")
    with open(p6, "wb") as f:
        f.write(b"P6\n# a comment\n5 7\n255\n" + img.tobytes())
    assert np.array_equal(lib.load_ppm(p6), img)
    with open(p6, "wb") as f:  # (a pixel byte that looks like white space must not be skipped)
        f.write(b"P6 1 1 255\n" + bytes([10, 32, 9]))
    assert np.array_equal(lib.load_ppm(p6), np.array([[[10, 32, 9]]], np.uint8))


def test_ppm_errors(tmp_path):
    def status_of(data):
        path = str(tmp_path / "bad.ppm")
        with open(path, "wb") as f:
            f.write(data)
        with pytest.raises(lib.FireflyError) as e:
            lib.load_ppm(path)
        return e.value.status

    assert status_of(b"P5\n1 1\n255\n\x00") == T.FF_ERR_INVALID_ARG
    assert status_of(b"P6\n2 2\n65535\n" + b"\x00" * 24) == T.FF_ERR_INVALID_ARG
    assert status_of(b"P6\n0 2\n255\n") == T.FF_ERR_INVALID_ARG
    assert status_of(b"P6\n2 2\n255\n" + b"\x00" * 11) == T.FF_ERR_IO
    assert status_of(b"P3\n1 1\n255\n1 2\n") == T.FF_ERR_IO
    assert status_of(b"P3\n1 1\n255\n1 2 300\n") == T.FF_ERR_IO
    with pytest.raises(lib.FireflyError) as e:
        lib.load_ppm(str(tmp_path / "missing.ppm"))
    assert e.value.status == T.FF_ERR_IO


def test_rgb8_to_linear_is_the_display_eotf():
    b = np.arange(256, dtype=np.uint8)
    s = b.astype(np.float64) / 255.0
    eotf = np.where(s <= 0.04045, s / 12.92, ((s + 0.055) / 1.055) ** 2.4)
    assert np.array_equal(bits(lib.rgb8_to_linear(b, srgb=True)), bits(eotf.astype(np.float32)))
    assert np.array_equal(bits(lib.rgb8_to_linear(b, srgb=False)), bits(s.astype(np.float32)))
    img = np.random.default_rng(1).integers(0, 256, (3, 4, 3)).astype(np.uint8)
    assert np.array_equal(lib.rgb8_to_linear(img), eotf.astype(np.float32)[img])


# ---- scene file ---------------------------------------------------------------------------------------------------------------

SCENE = """
bxdf white diffuse albedo 1 1 1
bxdf lamp emitter color 1 1 1 intensity 2
texture wood planks.ppm srgb
texture sky maps/sky.hdr clamp nearest
texture plain plain.ppm
plane position 0 -1 0 rotation 90 0 0 scale 4 4 4 albedo_map wood scale 2 3 offset 0.5 0.25 bxdf white
plane bxdf lamp position 0 2 0
sphere radius 1 bxdf white albedo_map sky
plane albedo_map plain offset 0.125 0.5 position 1 2 3 scale 2 2 2 bxdf white
"""


def write_scene(tmp_path, text):
    path = str(tmp_path / "scene.ff")
    with open(path, "w") as f:
        f.write(text)
    return path


def test_scene_file_textures_and_albedo_maps(tmp_path):
    sf = lib.SceneFile(write_scene(tmp_path, SCENE))
    try:
        assert len(sf) == 4
        tex = sf.textures()
        assert [t[0] for t in tex] == ["wood", "sky", "plain"]
        assert tex[0][1] == str(tmp_path / "planks.ppm") and tex[1][1] == str(tmp_path / "maps" / "sky.hdr")
        assert tex[0][2] == T.SCENE_TEX_SRGB and tex[1][2] == (T.TEX_CLAMP | T.TEX_NEAREST) and tex[2][2] == 0
        assert sf.albedo_map(0) == (0, (2.0, 3.0), (0.5, 0.25))
        assert sf.albedo_map(1) is None
        assert sf.albedo_map(2) == (1, (1.0, 1.0), (0.0, 0.0))
        assert sf.albedo_map(3) == (2, (1.0, 1.0), (0.125, 0.5))
        assert sf.albedo_map(4) is None and sf.albedo_map(-1) is None
        g = sf.geometries[3]  # (the geometry's own scale is still its own)
        assert (g.m_scale.x, g.m_scale.y, g.m_scale.z) == (2.0, 2.0, 2.0) and (g.m_position.x, g.m_position.z) == (1.0, 3.0)
        g = sf.geometries[0]
        assert (g.m_scale.x, g.m_scale.y, g.m_scale.z) == (4.0, 4.0, 4.0)
    finally:
        sf.close()


@pytest.mark.parametrize("text", [
    "bxdf w diffuse albedo 1 1 1\nplane bxdf w albedo_map nothing\n",                                  # a texture name not defined
    "bxdf w diffuse albedo 1 1 1\nplane bxdf w albedo_map\n",                                          # no name
    "bxdf w diffuse albedo 1 1 1\ntexture a a.ppm\ntexture a b.ppm\nplane bxdf w\n",                    # a duplicate name
    "bxdf w diffuse albedo 1 1 1\ntexture a\nplane bxdf w\n",                                          # no file
    "bxdf w diffuse albedo 1 1 1\ntexture a a.png\nplane bxdf w\n",                                    # neither .hdr nor .ppm
    "bxdf w diffuse albedo 1 1 1\ntexture a a.ppm mirror\nplane bxdf w\n",                             # an unknown option
    "bxdf w diffuse albedo 1 1 1\ntexture a a.ppm\nplane bxdf w albedo_map a scale 2\n",               # scale needs two numbers
    "bxdf w diffuse albedo 1 1 1\nplane bxdf w albedo_map a\ntexture a a.ppm\n",                       # used before its statement
])
def test_scene_file_texture_errors(tmp_path, text):
    with pytest.raises(lib.FireflyError) as e:
        lib.SceneFile(write_scene(tmp_path, text))
    assert e.value.status == T.FF_ERR_IO


def test_scene_file_without_textures(tmp_path):
    sf = lib.SceneFile(write_scene(tmp_path, "bxdf w diffuse albedo 1 1 1\nplane bxdf w\n"))
    try:
        assert sf.textures() == [] and sf.albedo_map(0) is None
    finally:
        sf.close()
