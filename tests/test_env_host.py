"""Environment light on the host (no GPU): the sampling table against numpy float64, the argument checks, the .hdr reader against
files written here, and the scene file's environment statement."""
import os

import numpy as np
import pytest

from gpupathtracer_amd import lib, scenes
from gpupathtracer_amd import types as T
import env_ref


def _maps():
    rng = np.random.default_rng(7)
    out = {
        "random": rng.random((16, 32, 3)).astype(np.float32),
        "random_wide": (rng.random((5, 13, 3)) ** 4 * 100).astype(np.float32),
        "hot_texel": np.zeros((8, 16, 3), np.float32),
        "one_by_one": np.array([[[0.5, 2.0, 1.0]]], np.float32),
        "w1": rng.random((9, 1, 3)).astype(np.float32),
        "h1": rng.random((1, 11, 3)).astype(np.float32),
        "sun_sky": scenes.sun_sky_map(64, 32),
    }
    out["hot_texel"][3, 5] = (10.0, 20.0, 5.0)
    z = rng.random((12, 10, 3)).astype(np.float32)
    z[[0, 4, 11]] = 0.0  # zero rows (the poles among them)
    out["zero_rows"] = z
    return out


MAPS = _maps()


@pytest.mark.parametrize("name", sorted(MAPS))
def test_table_matches_float64(ff, name):
    rgb = MAPS[name]
    tab = lib.environment_table(rgb)
    p, pdf = env_ref.table(rgb)
    assert np.allclose(tab["probability"], p, rtol=1e-6, atol=0.0)
    assert np.allclose(tab["pdf"], pdf, rtol=1e-6, atol=0.0)
    assert abs(tab["probability"].astype(np.float64).sum() - 1.0) < 1e-5
    # the alias table draws every texel with its probability
    assert np.allclose(env_ref.alias_probabilities(tab), p, rtol=1e-5, atol=1e-9)
    assert tab["alias"].min() >= 0 and tab["alias"].max() < rgb.shape[0] * rgb.shape[1]
    assert np.all((tab["alias_probability"] >= 0.0) & (tab["alias_probability"] <= 1.0))
    # a texel of zero luminance is never drawn
    black = (rgb.astype(np.float64) @ env_ref.LUM) == 0.0
    assert np.all(tab["pdf"][black] == 0.0)


def test_hot_texel_takes_every_sample(ff):
    tab = lib.environment_table(MAPS["hot_texel"])
    k = 3 * 16 + 5
    assert tab["probability"].ravel()[k] == 1.0
    ap, al = tab["alias_probability"].ravel(), tab["alias"].ravel()
    assert np.all((np.arange(ap.size) == k) | ((ap == 0.0) & (al == k)))
    assert np.isclose(tab["pdf"].ravel()[k], 1.0 / env_ref.solid_angles(16, 8)[3], rtol=1e-6)


def test_solid_angles_cover_the_sphere():
    for w, h in [(1, 1), (7, 3), (64, 32)]:
        assert np.isclose(env_ref.solid_angles(w, h).sum() * w, 4.0 * np.pi)


def test_all_zero_map_is_an_empty_table(ff):
    rgb = np.zeros((4, 8, 3), np.float32)
    tab = lib.environment_table(rgb)
    assert np.all(tab["probability"] == 0.0) and np.all(tab["pdf"] == 0.0)
    assert np.all(tab["alias_probability"] == 1.0)
    assert np.array_equal(tab["alias"].ravel(), np.arange(32))


@pytest.mark.parametrize("bad", ["nan", "inf", "negative", "neg_zero_ok"])
def test_table_rejects_bad_texels(ff, bad):
    rgb = np.ones((4, 4, 3), np.float32)
    rgb[2, 1, 1] = {"nan": np.nan, "inf": np.inf, "negative": -1e-30, "neg_zero_ok": -0.0}[bad]
    if bad == "neg_zero_ok":
        lib.environment_table(rgb)
        return
    with pytest.raises(lib.FireflyError) as e:
        lib.environment_table(rgb)
    assert e.value.status == T.FF_ERR_INVALID_ARG


def test_table_rejects_bad_sizes(ff):
    h = ff.load()
    buf = np.ones(12, np.float32)
    for w, hh in [(0, 1), (1, 0), (-3, 4), (1 << 13, (1 << 13) + 1)]:
        assert h.ff_environment_table(buf.ctypes.data, w, hh, None, None, None, None) == T.FF_ERR_INVALID_ARG
    assert h.ff_environment_table(None, 2, 2, None, None, None, None) == T.FF_ERR_INVALID_ARG
    assert h.ff_environment_table(buf.ctypes.data, 2, 2, None, None, None, None) == T.FF_OK


def test_set_environment_checks_its_arguments_without_a_gpu(ff):
    # (the checks come before the state is used: a null state is refused first, whatever the map)
    h = ff.load()
    rgb = np.ones((2, 4, 3), np.float32)
    assert h.ff_set_environment(None, rgb.ctypes.data, 4, 2, 1.0, 0.0) == T.FF_ERR_INVALID_ARG


# ---- Radiance .hdr files ----------------------------------------------------------------------------------------------------

def _rgbe_sample(h, w, seed=3):
    rng = np.random.default_rng(seed)
    vals = (rng.random((h, w, 3)) ** 3 * np.exp(rng.normal(0, 4, (h, w, 1)))).astype(np.float64)
    vals[0, : w // 2] = 0.0  # (a black run)
    vals[h - 1, :] = (0.25, 0.5, 1.0)  # (a run of one colour)
    q = env_ref.to_rgbe(vals)
    q[-1, 0] = (255, 255, 255, 255)  # largest exponent
    q[0, -1] = (1, 0, 128, 1)        # smallest
    return q


@pytest.mark.parametrize("rle", [False, True])
@pytest.mark.parametrize("shape", [(7, 40), (3, 8), (2, 5), (1, 1), (5, 300)])
def test_load_hdr_decodes_exactly(ff, tmp_path, rle, shape):
    q = _rgbe_sample(*shape)
    path = tmp_path / "map.hdr"
    path.write_bytes(env_ref.hdr_bytes(q, rle=rle))
    got = lib.load_hdr(str(path))
    assert got.dtype == np.float32 and got.shape == shape + (3,)
    assert np.array_equal(got.view(np.uint32), env_ref.decode_rgbe(q).view(np.uint32))


def test_load_hdr_mixed_scanlines_and_rgbe_signature(ff, tmp_path):
    # a file may mix run-length encoded and flat scanlines, and may start with #?RGBE and carry no FORMAT line
    q = _rgbe_sample(4, 16)
    data = bytearray(b"#?RGBE\n# a comment\n\n-Y 4 +X 16\n")
    for y in range(4):
        data += env_ref.hdr_bytes(q[y:y + 1], rle=(y % 2 == 0), header=b"#?RADIANCE\n\n").split(b"-Y 1 +X 16\n", 1)[1]
    path = tmp_path / "mixed.hdr"
    path.write_bytes(bytes(data))
    assert np.array_equal(lib.load_hdr(str(path)), env_ref.decode_rgbe(q))


def test_load_hdr_round_trips_a_sky(ff, tmp_path):
    sky = scenes.sun_sky_map(64, 32)
    path = tmp_path / "sky.hdr"
    path.write_bytes(env_ref.hdr_bytes(env_ref.to_rgbe(sky)))
    got = lib.load_hdr(str(path))
    # (8-bit mantissas under the texel's largest channel's exponent)
    assert np.all(np.abs(got - sky) <= sky.max(-1, keepdims=True) * 2.0 ** -7)


@pytest.mark.parametrize("case", ["missing", "no_signature", "no_blank_line", "bad_format", "bad_orientation", "zero_size",
                                  "truncated_flat", "truncated_rle", "run_overflow", "width_mismatch", "zero_count", "too_large"])
def test_load_hdr_errors(ff, tmp_path, case):
    q = _rgbe_sample(4, 16)
    good = env_ref.hdr_bytes(q, rle=True)
    head = b"#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n\n"
    data = {
        "no_signature": b"RADIANCE\n\n-Y 1 +X 1\n\x80\x80\x80\x80",
        "no_blank_line": b"#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n",
        "bad_format": b"#?RADIANCE\nFORMAT=32-bit_rle_xyze\n\n-Y 1 +X 1\n\x80\x80\x80\x80",
        "bad_orientation": head + b"+Y 1 +X 1\n\x80\x80\x80\x80",
        "zero_size": head + b"-Y 0 +X 4\n",
        "truncated_flat": env_ref.hdr_bytes(q, rle=False)[:-3],
        "truncated_rle": good[:-2],
        "run_overflow": head + b"-Y 1 +X 8\n" + bytes([2, 2, 0, 8, 128 + 9, 1]),
        "width_mismatch": head + b"-Y 1 +X 8\n" + bytes([2, 2, 0, 9]) + bytes(64),
        "zero_count": head + b"-Y 1 +X 8\n" + bytes([2, 2, 0, 8, 0]),
        "too_large": head + b"-Y 16384 +X 8192\n",
    }.get(case)
    path = tmp_path / "bad.hdr"
    if data is not None:
        path.write_bytes(data)
    with pytest.raises(lib.FireflyError) as e:
        lib.load_hdr(str(path))
    io = case in ("missing", "no_blank_line", "truncated_flat", "truncated_rle")
    assert e.value.status == (T.FF_ERR_IO if io else T.FF_ERR_INVALID_ARG), str(e.value)
    assert str(e.value)


# ---- scene file -------------------------------------------------------------------------------------------------------------

def _scene_file(tmp_path, env_line, sub="scenes"):
    d = tmp_path / sub
    d.mkdir(exist_ok=True)
    p = d / "open.scene"
    p.write_text("bxdf grey diffuse albedo 0.6 0.6 0.6\nplane position 0 -2.5 0 rotation 90 0 0 scale 40 40 40 bxdf grey\n" + env_line + "\n")
    return p


def test_scene_file_environment_statement(ff, tmp_path):
    p = _scene_file(tmp_path, "environment maps/sky.hdr intensity 2.5 rotation -30  # a comment")
    sf = lib.SceneFile(str(p))
    path, inten, rot = sf.environment()
    assert path == os.path.join(str(tmp_path / "scenes"), "maps/sky.hdr")
    assert inten == 2.5 and rot == -30.0
    sf.close()
    sf = lib.SceneFile(str(_scene_file(tmp_path, "environment /abs/sky.hdr rotation 90", sub="b")))
    assert sf.environment() == ("/abs/sky.hdr", 1.0, 90.0)
    sf = lib.SceneFile(str(_scene_file(tmp_path, "environment sky.hdr", sub="c")))
    assert sf.environment() == (str(tmp_path / "c" / "sky.hdr"), 1.0, 0.0)
    sf = lib.SceneFile(str(_scene_file(tmp_path, "", sub="d")))
    assert sf.environment() is None


def test_scene_file_environment_loads_with_the_reader(ff, tmp_path):
    sky = scenes.sun_sky_map(32, 16)
    (tmp_path / "scenes").mkdir()
    (tmp_path / "scenes" / "sky.hdr").write_bytes(env_ref.hdr_bytes(env_ref.to_rgbe(sky)))
    sf = lib.SceneFile(str(_scene_file(tmp_path, "environment sky.hdr intensity 0.5")))
    path, inten, _ = sf.environment()
    assert lib.load_hdr(path).shape == (16, 32, 3) and inten == 0.5


@pytest.mark.parametrize("line", ["environment", "environment sky.hdr intensity", "environment sky.hdr intensity -1",
                                  "environment sky.hdr intensity nan", "environment sky.hdr rotation x", "environment sky.hdr gamma 2",
                                  "environment a.hdr\nenvironment b.hdr"])
def test_scene_file_rejects_bad_environment_statements(ff, tmp_path, line):
    with pytest.raises(lib.FireflyError) as e:
        lib.SceneFile(str(_scene_file(tmp_path, line)))
    assert e.value.status == T.FF_ERR_IO


# ---- helpers ------------------------------------------------------------------------------------------------------------------

def test_sun_sky_map_is_deterministic_and_has_a_sun():
    a, b = scenes.sun_sky_map(128, 64), scenes.sun_sky_map(128, 64)
    assert a.dtype == np.float32 and a.shape == (64, 128, 3) and np.array_equal(a, b)
    lum = a.astype(np.float64) @ env_ref.LUM
    assert lum.max() > 1000.0 * np.median(lum)
    assert 1 <= (lum > 100.0).sum() <= 64
    r, c = env_ref.texel_of(np.array([0.35, 0.75, -0.55]) / np.linalg.norm([0.35, 0.75, -0.55]), 128, 64)
    assert lum[r, c] == lum.max()


def test_env_directions_map_to_their_texels():
    d = scenes.env_directions(24, 12)
    r, c = env_ref.texel_of(d, 24, 12)
    assert np.array_equal(r, np.repeat(np.arange(12)[:, None], 24, 1)) and np.array_equal(c, np.repeat(np.arange(24)[None, :], 12, 0))
    r90, c90 = env_ref.texel_of(d, 24, 12, 90.0)
    assert np.array_equal(c90, (c - 6) % 24)
