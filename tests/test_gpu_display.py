"""ff_display on the GPU: CLAMP + LINEAR is ff_render's own quantisation; display_out, rgb8 and the histogram agree bit for bit with
the numpy float32 reference (tests/display_ref.py) over image sizes, curves, encodings, bloom depths and inputs, the exposure
within display_ref.EXPOSURE_RTOL; buffer kinds and aliasing; temporal adaptation and its reset; non-finite pixels; isolation from
the other entry points; ff_display_to_pbo without a registered buffer."""
import ctypes as C
import functools

import numpy as np
import pytest

from gpupathtracer_amd import lib, scenes
from gpupathtracer_amd import types as T
from cases import build_case
import display_ref as R

pytestmark = pytest.mark.gpu

F = np.float32
AUTO, BLOOM = T.DISPLAY_AUTO_EXPOSURE, T.DISPLAY_BLOOM
SIZES = [(1, 1), (1, 7), (5, 3), (17, 9), (64, 64), (101, 67), (1920, 1080)]
CURVES = [T.CURVE_CLAMP, T.CURVE_REINHARD, T.CURVE_ACES]
ENCODINGS = [T.ENCODE_LINEAR, T.ENCODE_SRGB]
BLOOMS = [0, 1, 3, 8]  # 0: the flag off
C2_POSE = dict(position=(0.0, 0.0, 2.4), yaw=-90.0, pitch=0.0)
OPEN_POSE = dict(position=(0.0, -1.2, 3.0), yaw=-90.0, pitch=0.0)


def close(a, b):
    return abs(float(a) - float(b)) <= R.EXPOSURE_RTOL * abs(float(b))


@functools.lru_cache(maxsize=None)
def thresholds():
    return lib.srgb_thresholds()


@functools.lru_cache(maxsize=None)
def radiance(kind, w, h):
    """The three inputs of the parity tests at w x h: a rendered C2 frame, a rendered sun-and-sky frame, log-uniform noise.  Frames
    are rendered at no less than 16 x 16 and cropped (a 1 x 1 image of a frame is its top-left pixel)."""
    if kind == "random":
        rng = np.random.default_rng(1000 * w + h)
        return np.exp2(rng.uniform(-20.0, 20.0, (h, w, 3))).astype(np.float32)
    rw, rh = max(w, 16), max(h, 16)
    with lib.Tracer(0) as t:
        if kind == "c2":
            t.upload_scene(scenes.cornell_wahoo_scene())
            rad = t.render(scenes.posed_camera(rw, rh, **C2_POSE), lib.render_params(rw, rh, 6, 2, 99))[1]
        else:
            t.upload_scene(scenes.open_floor_scene())
            t.set_environment(scenes.sun_sky_map(256, 128))
            rad = t.render(scenes.posed_camera(rw, rh, **OPEN_POSE), lib.render_params(rw, rh, 3, 2, 7, shade_mode=T.SHADE_DIFFUSE_PATH_NEE))[1]
    return np.ascontiguousarray(rad[:h, :w])


def params(curve, encoding, bloom, auto=True, **more):
    flags = (AUTO if auto else 0) | (BLOOM if bloom else 0)
    return lib.display_params(curve=curve, encoding=encoding, flags=flags, bloom_levels=bloom if bloom else 5, **more)


def check_against_reference(tracer, rad, p, ep_cache=None, key=None):
    """One ff_display call without a previous exposure (an image without a countable pixel falls back to p.exposure) against the
    reference; returns the library's outputs."""
    tracer.display_reset()
    rgb8, out = tracer.display(rad, p)
    e, target, hist = tracer.display_state()
    if p.flags & AUTO:
        assert np.array_equal(hist, R.histogram(rad))
        rt, re_ = R.exposure(p, hist)
        assert close(target, rt) and close(e, re_), (target, rt, e, re_)
    else:
        assert not hist.any() and e == target == p.exposure
    # the reference goes on with the library's E: nothing downstream inherits the exposure's tolerance
    ep = None
    if ep_cache is not None:
        if (key, e) not in ep_cache:
            ep_cache[(key, e)] = R.exposed(rad, p, e)
        ep = ep_cache[(key, e)]
    ref8, ref_out = R.display(rad, p, e, thresholds(), ep)
    assert np.array_equal(R.bits(out), R.bits(ref_out)), f"{(R.bits(out) != R.bits(ref_out)).sum()} display_out values differ"
    assert np.array_equal(rgb8, ref8), f"{(rgb8 != ref8).sum()} bytes differ"
    return rgb8, out


def test_clamp_linear_is_ff_renders_own_quantisation(tracer):
    scene, cam, prm = build_case("path_cornell_96x64_b4_s4")
    tracer.upload_scene(scene)
    rgb8, rad = tracer.render(cam, prm)
    p = lib.display_params(curve=T.CURVE_CLAMP, encoding=T.ENCODE_LINEAR, flags=0, exposure=1.0)
    got8, out = tracer.display(rad, p)
    assert np.array_equal(got8, rgb8)
    assert np.array_equal(R.bits(out), R.bits(np.clip(rad, F(0), F(1)) + F(0)))
    assert rad.max() > 1 and (rgb8 == 255).any()  # (the frame does clip: the light is brighter than 1)
    e, target, hist = tracer.display_state()
    assert e == target == 1.0 and not hist.any()
    # only the bytes, only the floats, neither
    assert np.array_equal(tracer.display(rad, p, want_out=False)[0], rgb8)
    assert np.array_equal(R.bits(tracer.display(rad, p, want_rgb8=False)[1]), R.bits(out))
    assert tracer.display(rad, p, want_rgb8=False, want_out=False) == (None, None)


@pytest.mark.parametrize("kind", ["c2", "sun_sky", "random"])
@pytest.mark.parametrize("w,h", SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
def test_reference_parity_bit_for_bit(tracer, w, h, kind):
    rad = radiance(kind, w, h)
    cache = {}
    for bloom in BLOOMS:
        for curve in CURVES:
            for encoding in ENCODINGS:
                check_against_reference(tracer, rad, params(curve, encoding, bloom), cache, bloom)
    # manual exposure, a strong bloom with a low threshold, another white point and compensation
    check_against_reference(tracer, rad, params(T.CURVE_REINHARD, T.ENCODE_SRGB, 3, auto=False, exposure=0.37, white=1.5, bloom_threshold=0.1,
                                                bloom_strength=0.8))
    check_against_reference(tracer, rad, params(T.CURVE_ACES, T.ENCODE_SRGB, 8, exposure=2.5, key=0.3, low_percentile=0.1, high_percentile=1.0,
                                                bloom_threshold=0.0, bloom_strength=2.0))
    check_against_reference(tracer, rad, params(T.CURVE_ACES, T.ENCODE_SRGB, 2, bloom_strength=0.0))


def test_the_sun_and_sky_frame_is_neither_white_nor_black_any_more(tracer):
    """What the operator is for: ff_render's bytes of the sun-and-sky frame clip, the automatically exposed ACES + sRGB frame has
    a spread of mid-tones."""
    rad = radiance("sun_sky", 101, 67)
    naive = tracer.display(rad, lib.display_params(curve=T.CURVE_CLAMP, encoding=T.ENCODE_LINEAR))[0]
    shown = tracer.display(rad, lib.display_params(flags=AUTO))[0]
    mid = lambda a: float(((a > 16) & (a < 240)).mean())  # noqa: E731
    assert mid(shown) > 0.6 and mid(shown) > mid(naive) + 0.2, (mid(naive), mid(shown))


def test_buffer_kinds_aliasing_and_repeatability(tracer):
    import torch
    w, h = 101, 67
    rad = radiance("c2", w, h)
    for p in (params(T.CURVE_ACES, T.ENCODE_SRGB, 3), params(T.CURVE_REINHARD, T.ENCODE_LINEAR, 0, auto=False, exposure=1.7)):
        host8, host_out = tracer.display(rad, p)
        state = tracer.display_state()
        again8, again_out = tracer.display(rad, p)
        assert np.array_equal(host8, again8) and np.array_equal(R.bits(host_out), R.bits(again_out))
        d_rad = torch.from_numpy(rad).cuda()
        d8 = torch.zeros((h, w, 3), dtype=torch.uint8, device="cuda")
        d_out = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        tracer.display_device(w, h, d_rad.data_ptr(), p, d8.data_ptr(), d_out.data_ptr())
        assert np.array_equal(d8.cpu().numpy(), host8) and np.array_equal(R.bits(d_out.cpu().numpy()), R.bits(host_out))
        assert np.array_equal(R.bits(d_rad.cpu().numpy()), R.bits(rad))  # (the input is left alone)
        s2 = tracer.display_state()
        assert s2[:2] == state[:2] and np.array_equal(s2[2], state[2])
        # display_out on top of the input
        d8.zero_()
        tracer.display_device(w, h, d_rad.data_ptr(), p, d8.data_ptr(), d_rad.data_ptr())
        assert np.array_equal(d8.cpu().numpy(), host8) and np.array_equal(R.bits(d_rad.cpu().numpy()), R.bits(host_out))
        # buffers that are not 16-byte aligned (the kernels' scalar path), and an output that overlaps the input one pixel on
        big = torch.zeros(h * w * 3 + 16, dtype=torch.float32, device="cuda")
        big[1:1 + h * w * 3] = torch.from_numpy(rad).cuda().reshape(-1)
        b8 = torch.zeros(h * w * 3 + 8, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        tracer.display_device(w, h, big.data_ptr() + 4, p, b8.data_ptr() + 1, big.data_ptr() + 16)
        assert np.array_equal(b8.cpu().numpy()[1:1 + h * w * 3].reshape(h, w, 3), host8)
        assert np.array_equal(R.bits(big.cpu().numpy()[4:4 + h * w * 3].reshape(h, w, 3)), R.bits(host_out))
        # mixed: a device input with host outputs through the raw entry point
        lib_ = lib.load()
        m8, m_out = np.zeros((h, w, 3), np.uint8), np.zeros((h, w, 3), np.float32)
        d_rad = torch.from_numpy(rad).cuda()
        torch.cuda.synchronize()
        lib.check(lib_.ff_display(tracer._state, w, h, C.byref(p), C.c_void_p(d_rad.data_ptr()), 1, m8.ctypes.data, 0, m_out.ctypes.data, 0))
        assert np.array_equal(m8, host8) and np.array_equal(R.bits(m_out), R.bits(host_out))


def test_adaptation_follows_the_reference_and_reset_jumps(tracer):
    w, h = 64, 64
    base = radiance("c2", w, h)
    gains = [1.0, 8.0, 8.0, 0.05, 0.05, 3.0]
    p = lib.display_params(flags=AUTO | BLOOM, dt=1 / 60, bloom_levels=3)
    tracer.display_reset()
    prev = 0.0
    seen = []
    for i, g in enumerate(gains):
        rad = base * F(g)
        rgb8, out = tracer.display(rad, p)
        e, target, hist = tracer.display_state()
        assert np.array_equal(hist, R.histogram(rad))
        rt, re_ = R.exposure(p, hist, F(prev))
        assert close(target, rt) and close(e, re_), (i, target, rt, e, re_)
        if i == 0:
            assert e == target  # (nothing to adapt from)
        else:
            assert min(prev, target) <= e <= max(prev, target) and (e != target or prev == target)
        ref8, ref_out = R.display(rad, p, e, thresholds())
        assert np.array_equal(rgb8, ref8) and np.array_equal(R.bits(out), R.bits(ref_out))
        seen.append((e, target))
        prev = e
    assert seen[1][0] > seen[1][1] and seen[3][0] < seen[3][1]  # (brighter: the exposure is still above its target; darker: below)
    # a call without AUTO_EXPOSURE leaves the adapted exposure alone
    tracer.display(base, lib.display_params(exposure=0.5))
    assert tracer.display_state()[0] == 0.5
    tracer.display(base * F(gains[-1]), p)
    e, target, _ = tracer.display_state()
    assert close(e, R.exposure(p, R.histogram(base * F(gains[-1])), F(prev))[1]) and e != target
    # ... and a reset makes the next call jump
    tracer.display_reset()
    tracer.display(base * F(gains[-1]), p)
    e, target, _ = tracer.display_state()
    assert e == target
    # dt <= 0 does the same without a reset
    tracer.display(base * F(20.0), lib.display_params(flags=AUTO, dt=0.0))
    e, target, _ = tracer.display_state()
    assert e == target


def test_non_finite_pixels_spoil_only_themselves(tracer):
    w, h = 17, 9
    clean = radiance("random", w, h).copy() * F(2.0 ** -8)
    spots = [(2, 3), (5, 10), (8, 16)]
    bad = [(np.nan, 0.25, 0.5), (np.inf, np.inf, np.inf), (-np.inf, 0.5, np.nan)]
    dirty, black = clean.copy(), clean.copy()
    for (y, x), v in zip(spots, bad):
        dirty[y, x] = v
        black[y, x] = 0
    tracer.display_reset()
    for curve in CURVES:
        for levels in (1, 3, 8):
            p = params(curve, T.ENCODE_SRGB, levels, bloom_threshold=0.05, bloom_strength=1.0)
            b8, b_out = tracer.display(black, p)
            b_state = tracer.display_state()
            d8, d_out = tracer.display(dirty, p)
            d_state = tracer.display_state()
            assert d_state[:2] == b_state[:2] and np.array_equal(d_state[2], b_state[2])
            assert np.array_equal(d_state[2], R.histogram(dirty))
            mask = np.ones((h, w), bool)
            for y, x in spots:
                mask[y, x] = False
            assert np.array_equal(d8[mask], b8[mask]) and np.array_equal(R.bits(d_out[mask]), R.bits(b_out[mask]))
            # step 3: NaN -> 0, -Inf -> 0, +Inf -> 1; a finite channel goes the ordinary way (exposure and the neighbours' bloom)
            (y0, x0), (y1, x1), (y2, x2) = spots
            assert d8[y0, x0, 0] == 0 and d_out[y0, x0, 0] == 0
            assert d8[y1, x1].tolist() == [255, 255, 255] and d_out[y1, x1].tolist() == [1.0, 1.0, 1.0]
            assert d8[y2, x2, 0] == 0 and d8[y2, x2, 2] == 0 and d_out[y2, x2, 0] == 0 and d_out[y2, x2, 2] == 0
            ref8, ref_out = R.display(dirty, p, d_state[0], thresholds())
            assert np.array_equal(d8, ref8) and np.array_equal(R.bits(d_out), R.bits(ref_out))
            assert np.isfinite(d_out).all()


def test_display_is_not_a_frame(tracer):
    w, h = 96, 64
    scene = scenes.cornell_wahoo_scene()
    cam = scenes.posed_camera(w, h, **C2_POSE)
    prm = lib.render_params(w, h, 6, 1, 42)
    tracer.upload_scene(scene)
    tracer.taa_reset()
    tracer.temporal_reset()
    gb = tracer.gbuffer(cam, lib.render_params(w, h))
    first = tracer.render(cam, prm)
    second = tracer.render(cam, prm)           # (the camera is at rest: served from the stored primary hits)
    st = tracer.stats()
    tracer.denoise_temporal(second[1], gb, cam)
    tracer.taa(second[1], gb, cam)
    taa_hist, tp_hist = tracer.taa_history(), tracer.temporal_history()

    def snapshot():
        s = tracer.stats()
        return {f: getattr(s, f) for f, _ in s._fields_}
    before = snapshot()
    for p in (lib.display_params(flags=AUTO | BLOOM), lib.display_params(curve=T.CURVE_CLAMP, encoding=T.ENCODE_LINEAR)):
        tracer.display(second[1], p)
        tracer.display(radiance("random", 1920, 1080), p)  # (a larger image: the scratch buffers are regrown)
    assert snapshot() == before
    for a, b in zip(tracer.taa_history() + tracer.temporal_history(), taa_hist + tp_hist):
        assert np.array_equal(R.bits(a), R.bits(b))
    third = tracer.render(cam, prm)
    assert np.array_equal(third[0], second[0]) and np.array_equal(R.bits(third[1]), R.bits(second[1]))
    assert np.array_equal(R.bits(first[1]), R.bits(second[1]))
    s3 = tracer.stats()
    assert (s3.rays_answered, s3.rays_traced, s3.flags, s3.kernel_launches) == (st.rays_answered, st.rays_traced, st.flags, st.kernel_launches)
    # the filters continue from their histories as if nothing had happened in between
    with lib.Tracer(0) as other:
        other.upload_scene(scene)
        gb2 = other.gbuffer(cam, lib.render_params(w, h))
        r = other.render(cam, prm)[1]
        other.render(cam, prm)
        other.denoise_temporal(r, gb2, cam)
        other.taa(r, gb2, cam)
        want_tp, want_taa = other.denoise_temporal(r, gb2, cam), other.taa(r, gb2, cam)
    got_tp, got_taa = tracer.denoise_temporal(second[1], gb, cam), tracer.taa(second[1], gb, cam)
    for a, b in zip(got_tp + got_taa, want_tp + want_taa):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
    # ff_upload_scene does not reset the adapted exposure
    p = lib.display_params(flags=AUTO, dt=1 / 60)
    tracer.display_reset()
    tracer.display(second[1], p)
    e0 = tracer.display_state()[0]
    tracer.upload_scene(scene)
    tracer.display(second[1] * F(16), p)
    e1, t1, _ = tracer.display_state()
    assert t1 < e1 < e0


def test_argument_checks_come_before_any_device_work(tracer):
    lib_ = lib.load()
    rad = np.zeros((4, 4, 3), np.float32)
    out = np.full((4, 4, 3), 7.0, np.float32)
    tracer.display(rad, lib.display_params())
    before = tracer.display_state()

    def call(p, w=4, h=4, src=rad):
        return lib_.ff_display(tracer._state, w, h, C.byref(p) if p is not None else None, src.ctypes.data if src is not None else None, 0, None, 0,
                               out.ctypes.data, 0)
    for field, value in [("curve", 5), ("encoding", 7), ("flags", 8), ("exposure", 0.0), ("white", float("nan")), ("key", -1.0),
                         ("low_percentile", 1.0), ("high_percentile", 2.0), ("min_exposure", 0.0), ("max_exposure", 1e-9), ("adapt_darken", -1.0),
                         ("adapt_brighten", float("nan")), ("dt", float("nan")), ("bloom_threshold", -1.0), ("bloom_strength", float("inf")),
                         ("bloom_levels", 9)]:
        assert call(lib.display_params(**{field: value})) == T.FF_ERR_INVALID_ARG
        assert field in lib_.ff_last_error().decode()
    p = lib.display_params()
    assert call(None) == T.FF_ERR_INVALID_ARG and call(p, src=None) == T.FF_ERR_INVALID_ARG and b"radiance_in" in lib_.ff_last_error()
    for w, h in [(0, 4), (4, 0), (-1, 4), (4, 70000)]:
        assert call(p, w, h) == T.FF_ERR_INVALID_ARG and b"size" in lib_.ff_last_error()
    assert (out == 7.0).all()
    after = tracer.display_state()
    assert after[:2] == before[:2] and np.array_equal(after[2], before[2])


def test_display_to_pbo_needs_a_registered_buffer(tracer):
    rad = np.zeros((4, 4, 3), np.float32)
    with pytest.raises(lib.FireflyError) as e:
        tracer.display_to_pbo(rad)
    assert e.value.status == T.FF_ERR_GL_UNAVAILABLE and "no pixel buffer" in e.value.message


def test_display_state_before_the_first_call():
    with lib.Tracer(0) as t:
        with pytest.raises(lib.FireflyError) as e:
            t.display_state()
        assert e.value.status == T.FF_ERR_INVALID_ARG
        t.display_reset()
        # no scene is needed
        rgb8, out = t.display(np.full((3, 5, 3), 0.18, np.float32), lib.display_params(flags=AUTO))
        assert len(np.unique(rgb8)) == 1 and 100 < rgb8[0, 0, 0] < 160
