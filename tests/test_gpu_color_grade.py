"""ff_color_grade on the GPU: bit for bit, radiance and bytes, against the host twin and the numpy float32 restatement
(tests/color_grade_ref.py) at pixel counts around the lane's quad and the wave and at one beyond a pass of the persistent grid; LUT
sizes on both sides of the LDS dispatch and the curves that no longer fit beside the lattice; every kernel instantiation; non-finite
pixels beside the quad, wave and workgroup seams; in place and refused overlaps; buffer kinds; the LUT objects' life; isolation from
the other entry points; the shared work buffer; and the chain render -> ff_color_grade -> ff_display -> ff_encode_yuv."""
import contextlib
import ctypes as C

import numpy as np
import pytest

from gpupathtracer_amd import lib, scenes
from gpupathtracer_amd import types as T
import color_grade_ref as R
from color_grade_cases import (AXES, FLAG_SETTINGS, ONE_PASS_PIXELS, assert_same, flags_id, inputs, log_axis, make_lut, params, planted_non_finite)

pytestmark = pytest.mark.gpu

F = np.float32
C2_POSE = dict(yaw=-90.0, pitch=0.0)
SIZES = [(1, 1), (3, 1), (63, 1), (65, 3), (33, 9), (257, 5)]
LDS_N = T.GRADE_LDS_MAX_SIZE
ALL = R.PRIMARY | R.CURVES | R.LUT3D


@contextlib.contextmanager
def on_device(tracer, lut):
    lut_id = tracer.grade_lut_create(lut)
    try:
        yield lut_id
    finally:
        tracer.grade_lut_destroy(lut_id)


def check_all_three(tracer, rad, flags, lut, lut_id, restate=True):
    got = tracer.color_grade(rad, params(flags, lut_id))
    assert_same(got, lib.color_grade_host(rad, params(flags), lut))
    if restate:
        assert_same(got, R.color_grade(rad, params(flags), lut))
    return got


@pytest.mark.parametrize("size", SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
def test_device_twin_and_restatement_bit_for_bit(tracer, size):
    for axis in AXES:
        lut = make_lut(5, 129, axis)
        rad = inputs(*size, lut)
        with on_device(tracer, lut) as lut_id:
            for flags in FLAG_SETTINGS:
                check_all_three(tracer, rad, flags, lut, lut_id)


def test_more_quads_than_one_pass_of_the_grid():
    """The persistent grid holds GRADE_MAX_BLOCKS x GRADE_THREADS lanes of GRADE_PIXELS_PER_LANE pixels: this image has 123 quads
    more, so the grid-stride loop runs twice in the first workgroup, and its pixel count is no multiple of 4."""
    w, h = 1031, 509
    quads = -(-w * h // T.GRADE_PIXELS_PER_LANE)
    assert w * h > ONE_PASS_PIXELS and 0 < quads - T.GRADE_MAX_BLOCKS * T.GRADE_THREADS < T.GRADE_THREADS and (w * h) % 4
    with lib.Tracer(0) as t:   # (its own state: the session's work buffer stays small)
        lut = make_lut(LDS_N, 129, R.AXIS_LOG)
        rad = inputs(w, h, lut)
        with on_device(t, lut) as lut_id:
            check_all_three(t, rad, ALL, lut, lut_id)
            assert_same(t.color_grade(rad, params(0)), (R.to_u8(rad), rad))
        lut = make_lut(LDS_N + 1, 129, R.AXIS_LINEAR)
        with on_device(t, lut) as lut_id:
            check_all_three(t, rad, ALL | R.TRILINEAR, lut, lut_id, restate=False)


LUT_KEYS = [(2, 2), (2, 129), (LDS_N, 2), (LDS_N, 129), (LDS_N, 4096), (LDS_N + 1, 129), (LDS_N + 1, 4096), (33, 129), (65, 2)]


@pytest.mark.parametrize("key", LUT_KEYS, ids=[f"N{n}-K{k}" for n, k in LUT_KEYS])
def test_lut_sizes_on_both_sides_of_the_dispatch(tracer, key):
    N, K = key
    lut = make_lut(N, K, R.AXIS_LOG if K != 2 else R.AXIS_LINEAR)
    rad = inputs(257, 5, lut)
    with on_device(tracer, lut) as lut_id:
        for flags in (R.LUT3D, R.LUT3D | R.TRILINEAR, R.CURVES | R.LUT3D, ALL, ALL | R.TRILINEAR, R.CURVES):
            check_all_three(tracer, rad, flags, lut, lut_id)


def instantiation(flags, N, K, no_lds=False):
    """The key (PRIMARY, CURVES, LUT, HOME) of the kernel a call runs: the dispatch of ff_color_grade restated from types.py."""
    lattice, curves = bool(flags & R.LUT3D), bool(flags & R.CURVES)
    home = 0
    if lattice and N <= T.GRADE_LDS_MAX_SIZE and not no_lds:
        lattice_bytes = (N ** 3 * 12 + 15) & ~15
        home = 1 if lattice_bytes + (12 * K if curves else 0) <= T.GRADE_LDS_BYTES else 2
    return bool(flags & R.PRIMARY), curves, 0 if not lattice else (2 if flags & R.TRILINEAR else 1), home


# what csrc/ff_grade.hip instantiates: without a lattice one home; with one, two; with curves as well, three
INSTANTIATIONS = {(p, c, l, h) for p in (False, True) for c in (False, True) for l in (0, 1, 2) for h in (0, 1, 2)
                  if h == 0 or (l != 0 and (h == 1 or c))}


def test_every_instantiation_is_reached(tracer, monkeypatch):
    assert len(INSTANTIATIONS) == 24
    reached = set()
    luts = [make_lut(LDS_N, 129, R.AXIS_LINEAR), make_lut(LDS_N, 4096, R.AXIS_LOG), make_lut(LDS_N + 1, 129, R.AXIS_LINEAR)]
    rad = inputs(65, 3, luts[0])
    results = {}
    for n, lut in enumerate(luts):
        with on_device(tracer, lut) as lut_id:
            for flags in FLAG_SETTINGS:
                results[n, flags] = check_all_three(tracer, rad, flags, lut, lut_id, restate=False)
                reached.add(instantiation(flags, lut.desc.size, lut.desc.curve_size))
    assert reached == INSTANTIATIONS
    # the LDS sizes once more with every lattice in global memory: the same bits
    monkeypatch.setenv("FF_GRADE_NO_LDS", "1")
    with lib.Tracer(0) as t:
        for n, lut in enumerate(luts[:2]):
            with on_device(t, lut) as lut_id:
                for flags in FLAG_SETTINGS:
                    assert instantiation(flags, lut.desc.size, lut.desc.curve_size, no_lds=True)[3] == 0
                    assert_same(t.color_grade(rad, params(flags, lut_id)), results[n, flags])


def test_non_finite_pixels_beside_the_seams(tracer):
    """257 x 5 = 1285 pixels: a lane's quad ends at pixel 3 | 4, a wave at 255 | 256, a workgroup at 1023 | 1024; 1284 is the one
    pixel of the last quad."""
    lut = make_lut(LDS_N, 129, R.AXIS_LOG)
    clean = inputs(257, 5, lut)
    places = (0, 3, 4, 255, 256, 259, 1023, 1024, 1284)
    bad = planted_non_finite(clean, places)
    mask = np.zeros(1285, bool)
    mask[list(places)] = True
    mask = mask.reshape(5, 257)
    with on_device(tracer, lut) as lut_id:
        for flags in FLAG_SETTINGS:
            rgb8, out = check_all_three(tracer, bad, flags, lut, lut_id)
            ref8, ref = tracer.color_grade(clean, params(flags, lut_id))
            assert np.array_equal(R.bits(out[mask]), R.bits(bad[mask])) and np.array_equal(rgb8[mask], R.to_u8(bad[mask])), flags_id(flags)
            assert np.array_equal(R.bits(out[~mask]), R.bits(ref[~mask])) and np.array_equal(rgb8[~mask], ref8[~mask]), flags_id(flags)
            assert np.isfinite(out[~mask]).all()


def test_buffer_kinds_in_place_and_aliasing(tracer):
    import torch
    w, h = 101, 67
    n = w * h * 3
    lut = make_lut(LDS_N, 129, R.AXIS_LINEAR)
    rad = inputs(w, h, lut)
    with on_device(tracer, lut) as lut_id:
        p = params(ALL, lut_id)
        host8, host_out = check_all_three(tracer, rad, ALL, lut, lut_id)
        # only the bytes, only the floats, neither; in place on the host
        got = tracer.color_grade(rad, p, want_out=False)
        assert got[1] is None and np.array_equal(got[0], host8)
        got = tracer.color_grade(rad, p, want_rgb8=False)
        assert got[0] is None and np.array_equal(R.bits(got[1]), R.bits(host_out))
        assert tracer.color_grade(rad, p, want_rgb8=False, want_out=False) == (None, None)
        assert_same(tracer.color_grade(rad, p, in_place=True), (host8, host_out))
        # a device tensor through the same method, then in place
        d_rad = torch.from_numpy(np.array(rad)).cuda()
        t8, t_out = tracer.color_grade(d_rad, p)
        assert t8.is_cuda and t_out.is_cuda
        assert_same((t8.cpu().numpy(), t_out.cpu().numpy()), (host8, host_out))
        assert np.array_equal(R.bits(d_rad.cpu().numpy()), R.bits(rad))  # (the input is left alone)
        d_copy = d_rad.clone()
        t8, t_out = tracer.color_grade(d_copy, p, in_place=True)
        assert t_out.data_ptr() == d_copy.data_ptr()
        assert_same((t8.cpu().numpy(), d_copy.cpu().numpy()), (host8, host_out))
        # raw pointers: one output at a time, then neither
        d8 = torch.zeros((h, w, 3), dtype=torch.uint8, device="cuda")
        d_out = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        src = d_rad.data_ptr()
        tracer.color_grade_device(w, h, src, p, d8.data_ptr(), None)
        assert np.array_equal(d8.cpu().numpy(), host8)
        tracer.color_grade_device(w, h, src, p, None, d_out.data_ptr())
        assert np.array_equal(R.bits(d_out.cpu().numpy()), R.bits(host_out))
        tracer.color_grade_device(w, h, src, p, None, None)
        # buffers that are only 4-byte (1-byte) aligned, with guard words on both sides of the outputs; then in place there
        big = torch.zeros(n + 8, dtype=torch.float32, device="cuda")
        big[1:1 + n] = d_rad.reshape(-1)
        big_out = torch.full((n + 8,), 7.0, dtype=torch.float32, device="cuda")
        b8 = torch.full((n + 8,), 7, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        tracer.color_grade_device(w, h, big.data_ptr() + 4, p, b8.data_ptr() + 1, big_out.data_ptr() + 4)
        assert np.array_equal(b8.cpu().numpy()[1:1 + n].reshape(h, w, 3), host8)
        assert np.array_equal(R.bits(big_out.cpu().numpy()[1:1 + n].reshape(h, w, 3)), R.bits(host_out))
        guard_f, guard_b = big_out.cpu().numpy(), b8.cpu().numpy()
        assert guard_f[0] == 7.0 and (guard_f[1 + n:] == 7.0).all() and guard_b[0] == 7 and (guard_b[1 + n:] == 7).all()
        tracer.color_grade_device(w, h, big.data_ptr() + 4, p, None, big.data_ptr() + 4)
        guard_f = big.cpu().numpy()
        assert np.array_equal(R.bits(guard_f[1:1 + n].reshape(h, w, 3)), R.bits(host_out)) and guard_f[0] == 0.0 and (guard_f[1 + n:] == 0.0).all()
        # mixed: a device input with host outputs, a host input with device outputs, through the raw entry point
        lib_ = lib.load()
        m8, m_out = np.zeros((h, w, 3), np.uint8), np.zeros((h, w, 3), np.float32)
        vp = C.c_void_p
        lib.check(lib_.ff_color_grade(tracer._state, C.byref(p), w, h, vp(src), 1, m8.ctypes.data, 0, m_out.ctypes.data, 0))
        assert_same((m8, m_out), (host8, host_out))
        d8.zero_()
        d_out.zero_()
        torch.cuda.synchronize()
        lib.check(lib_.ff_color_grade(tracer._state, C.byref(p), w, h, rad.ctypes.data, 0, vp(d8.data_ptr()), 1, vp(d_out.data_ptr()), 1))
        assert_same((d8.cpu().numpy(), d_out.cpu().numpy()), (host8, host_out))
        # any overlap but radiance_out == radiance_in is refused on the host: nothing is launched, nothing is written
        d_out.fill_(7.0)
        torch.cuda.synchronize()
        dst = d_out.data_ptr()
        for args, words in [((None, src + 4), "radiance_out overlaps radiance_in"), ((None, src - 4 * n + 4), "radiance_out overlaps radiance_in"),
                            ((None, src + 4 * n - 4), "radiance_out overlaps radiance_in"), ((src + 16, None), "rgb8 overlaps radiance_in"),
                            ((src - n + 1, None), "rgb8 overlaps radiance_in"), ((src, src), "rgb8 overlaps radiance_in"),
                            ((dst + 64, dst), "rgb8 overlaps radiance_out"), ((dst + 4 * n - 1, dst), "rgb8 overlaps radiance_out")]:
            with pytest.raises(lib.FireflyError) as e:
                tracer.color_grade_device(w, h, src, p, *args)
            assert e.value.status == T.FF_ERR_INVALID_ARG and words in e.value.message
        assert (d_out.cpu().numpy() == 7.0).all()
        assert np.array_equal(R.bits(d_rad.cpu().numpy()), R.bits(rad))


def test_lut_lifecycle():
    a, b = make_lut(5, 129, R.AXIS_LOG), make_lut(LDS_N + 1, 3, R.AXIS_LINEAR)
    rad = inputs(65, 3, a)
    with lib.Tracer(0) as t:
        ida, idb = t.grade_lut_create(a), t.grade_lut_create(b)
        assert (ida, idb) == (0, 1)
        # two LUTs alternate between calls
        for lut, lut_id in ((a, ida), (b, idb), (a, ida), (b, idb)):
            assert_same(t.color_grade(rad, params(ALL, lut_id)), lib.color_grade_host(rad, params(ALL), lut))
        # LUTs survive an upload
        t.upload_scene(scenes.cornell_wahoo_scene())
        assert_same(t.color_grade(rad, params(ALL, ida)), lib.color_grade_host(rad, params(ALL), a))
        # a destroyed id is refused, then given out again
        t.grade_lut_destroy(ida)
        for call in (lambda: t.color_grade(rad, params(ALL, ida)), lambda: t.grade_lut_destroy(ida), lambda: t.grade_lut_destroy(-1),
                     lambda: t.grade_lut_destroy(16), lambda: t.color_grade(rad, params(0, 5)), lambda: t.color_grade(rad, params(ALL, -1)),
                     lambda: t.color_grade(rad, params(0, -2))):
            with pytest.raises(lib.FireflyError) as e:
                call()
            assert e.value.status == T.FF_ERR_INVALID_ARG and "lut" in e.value.message
        assert_same(t.color_grade(rad, params(ALL, idb)), lib.color_grade_host(rad, params(ALL), b))
        assert t.grade_lut_create(b) == ida
        assert_same(t.color_grade(rad, params(ALL, ida)), lib.color_grade_host(rad, params(ALL), b))
        # a stage whose half the LUT lacks
        only_curves = make_lut(0, 3, R.AXIS_LINEAR)
        idc = t.grade_lut_create(only_curves)
        assert idc == 2
        with pytest.raises(lib.FireflyError, match="no lattice"):
            t.color_grade(rad, params(R.LUT3D, idc))
        assert_same(t.color_grade(rad, params(R.CURVES, idc)), lib.color_grade_host(rad, params(R.CURVES), only_curves))
        # the 17th is refused; a refused descriptor takes no id
        ids = [t.grade_lut_create(only_curves) for _ in range(T.GRADE_MAX_LUTS - 3)]
        assert ids == list(range(3, T.GRADE_MAX_LUTS))
        with pytest.raises(lib.FireflyError, match="already holds 16"):
            t.grade_lut_create(only_curves)
        t.grade_lut_destroy(7)
        with pytest.raises(lib.FireflyError, match="curve_lo"):
            t.grade_lut_create(lib.grade_lut(curves=only_curves.curves, curve_lo=1.0, curve_hi=1.0))
        assert t.grade_lut_create(a) == 7
        assert_same(t.color_grade(rad, params(ALL, 7)), lib.color_grade_host(rad, params(ALL), a))


def test_no_scene_is_needed_and_arguments_are_checked_first():
    lut = make_lut(3, 3, R.AXIS_LINEAR)
    rad = inputs(17, 15, lut)
    with lib.Tracer(0) as t:
        lut_id = t.grade_lut_create(lut)
        assert_same(t.color_grade(rad, params(ALL, lut_id)), lib.color_grade_host(rad, params(ALL), lut))
        out = np.full((15, 17, 3), 7.0, np.float32)
        lib_ = lib.load()
        for fields, word in [(dict(flags=16), "flags"), (dict(reserved=1), "reserved"), (dict(saturation=-1.0), "saturation"),
                             (dict(offset=(0, float("nan"), 0)), "offset[1]"), (dict(matrix=(float("inf"),) * 9), "matrix[0]"), (dict(lut_id=9), "lut_id 9"),
                             (dict(flags=R.CURVES), "lut_id -1")]:
            q = lib.grade_params(**fields)
            assert lib_.ff_color_grade(t._state, C.byref(q), 17, 15, rad.ctypes.data, 0, None, 0, out.ctypes.data, 0) == T.FF_ERR_INVALID_ARG
            assert word in lib_.ff_last_error().decode(), lib_.ff_last_error().decode()
        p = params(ALL, lut_id)
        assert lib_.ff_color_grade(t._state, None, 17, 15, rad.ctypes.data, 0, None, 0, out.ctypes.data, 0) == T.FF_ERR_INVALID_ARG
        assert "params" in lib_.ff_last_error().decode()
        assert lib_.ff_color_grade(None, C.byref(p), 17, 15, rad.ctypes.data, 0, None, 0, out.ctypes.data, 0) == T.FF_ERR_INVALID_ARG
        assert lib_.ff_color_grade(t._state, C.byref(p), 17, 15, None, 0, None, 0, out.ctypes.data, 0) == T.FF_ERR_INVALID_ARG
        assert "radiance_in" in lib_.ff_last_error().decode()
        for w, h in ((0, 15), (17, 65536)):
            assert lib_.ff_color_grade(t._state, C.byref(p), w, h, rad.ctypes.data, 0, None, 0, out.ctypes.data, 0) == T.FF_ERR_INVALID_ARG
            assert "image size" in lib_.ff_last_error().decode()
        assert (out == 7.0).all()


def test_color_grade_is_not_a_frame(tracer):
    w, h = 96, 64
    scene = scenes.cornell_wahoo_scene()
    cam = scenes.posed_camera(w, h, position=(0.0, 0.0, 2.4), **C2_POSE)
    prm = lib.render_params(w, h, 6, 1, 42)
    flat = lib.render_params(w, h)
    tracer.upload_scene(scene)
    tracer.taa_reset()
    tracer.temporal_reset()
    gb = tracer.gbuffer(cam, flat)
    first = tracer.render(cam, prm)
    second = tracer.render(cam, prm)           # (the camera is at rest: served from the stored primary hits)
    st, name = tracer.stats(), tracer.kernel_name()
    tracer.denoise_temporal(second[1], gb, cam)
    tracer.taa(second[1], gb, cam)
    tracer.display(second[1], lib.display_params(flags=T.DISPLAY_AUTO_EXPOSURE))
    taa_hist, tp_hist, disp = tracer.taa_history(), tracer.temporal_history(), tracer.display_state()

    def snapshot():
        s = tracer.stats()
        return {f: getattr(s, f) for f, _ in s._fields_}
    before = snapshot()
    lut = make_lut(LDS_N, 129, R.AXIS_LOG)
    with on_device(tracer, lut) as lut_id:
        check_all_three(tracer, second[1], ALL, lut, lut_id)
        tracer.color_grade(inputs(320, 180, lut), params(ALL | R.TRILINEAR, lut_id))  # (a larger image: the work buffer is regrown)
    assert snapshot() == before and tracer.kernel_name() == name
    for a, b in zip(tracer.taa_history() + tracer.temporal_history(), taa_hist + tp_hist):
        assert np.array_equal(R.bits(a), R.bits(b))
    after = tracer.display_state()
    assert after[:2] == disp[:2] and np.array_equal(after[2], disp[2])
    again = tracer.gbuffer(cam, flat)          # (at rest: the stored primary hits are still there and still this frame's)
    for key in gb:
        assert np.array_equal(np.asarray(again[key]).view(np.uint32), np.asarray(gb[key]).view(np.uint32)), key
    third = tracer.render(cam, prm)
    assert np.array_equal(third[0], second[0]) and np.array_equal(R.bits(third[1]), R.bits(second[1]))
    assert np.array_equal(R.bits(first[1]), R.bits(second[1]))
    s3 = tracer.stats()
    assert (s3.rays_answered, s3.rays_traced, s3.flags, s3.kernel_launches) == (st.rays_answered, st.rays_traced, st.flags, st.kernel_launches)


def test_the_work_buffer_is_shared_with_other_filters(tracer):
    """ff_color_grade between a larger ff_sharpen and a smaller ff_resize on one Tracer, host arrays each time: every call stages in
    the one image work buffer, and each equals its twin."""
    lut = make_lut(5, 129, R.AXIS_LINEAR)
    with on_device(tracer, lut) as lut_id:
        for _ in range(2):
            big = inputs(320, 180, lut)
            assert_same(tracer.sharpen(big), lib.sharpen_host(big))
            rad = inputs(101, 67, lut)
            assert_same(tracer.color_grade(rad, params(ALL, lut_id)), lib.color_grade_host(rad, params(ALL), lut))
            small = inputs(33, 9, lut)
            assert_same(tracer.resize(small, 20, 12), lib.resize_host(small, 20, 12))
            assert_same(tracer.color_grade(big, params(ALL, lut_id), in_place=True), lib.color_grade_host(big, params(ALL), lut))


def test_chain_on_a_real_frame(tracer):
    """A 1-spp 128 x 72 frame of the mirror Cornell box with next-event estimation, graded - a LOG shaper into a 17^3 lattice that
    desaturates -, shown and encoded: the kernel against the twin on what the path tracer really produces, finite, and not what the
    ungraded chain gives."""
    w, h = 128, 72
    tracer.upload_scene(scenes.cornell_mirror_scene())
    cam = scenes.posed_camera(w, h, position=(0.0, 0.0, 5.0), **C2_POSE)  # (from outside the open front: the light and misses are in view)
    rad = tracer.render(cam, lib.render_params(w, h, 8, 1, seed=11, shade_mode=T.SHADE_DIFFUSE_PATH_NEE))[1]
    assert np.isfinite(rad).all() and (rad >= 0).all() and rad.any()
    # the shaper: 8 knots to a binade over 2^-8 .. 2^8, y = (log2 x + 8) / 16; the lattice over 0 .. 1 in shaper space: half-way to grey
    lo, hi, shift = log_axis(129)
    y = np.linspace(0.0, 1.0, 129)
    g = np.linspace(0.0, 1.0, LDS_N)
    b, gg, r = np.meshgrid(g, g, g, indexing="ij")
    lum = 0.2126 * r + 0.7152 * gg + 0.0722 * b
    table = np.stack([0.5 * (c + lum) for c in (r, gg, b)], axis=-1)
    lut = lib.grade_lut(curves=np.stack([y, y, y]), curve_lo=lo, curve_hi=hi, curve_axis=R.AXIS_LOG, curve_shift=shift, table=table)
    with on_device(tracer, lut) as lut_id:
        p = lib.grade_params(flags=R.CURVES | R.LUT3D, lut_id=lut_id)
        rgb8, out = tracer.color_grade(rad, p)
    assert_same((rgb8, out), lib.color_grade_host(rad, p, lut))
    assert_same((rgb8, out), R.color_grade(rad, p, lut))
    eps = 16 * 2.0 ** -24   # (knots and texels lie in 0 .. 1; the formulas' roundings, test_color_grade_host.py)
    assert np.isfinite(out).all() and out.min() >= -eps and out.max() <= 1.0 + eps
    dp = lib.display_params(encoding=T.ENCODE_LINEAR)
    shown = tracer.display(out, dp)[1]
    plain = tracer.display(rad, dp)[1]
    assert shown.shape == (h, w, 3) and np.isfinite(shown).all() and not np.array_equal(shown, plain)
    luma, chroma = tracer.encode_yuv(shown)
    luma0, chroma0 = tracer.encode_yuv(plain)
    assert luma.shape == (h, w) and chroma.shape == (h // 2, w // 2, 2) and len(np.unique(luma)) > 8
    assert not np.array_equal(luma, luma0) and not np.array_equal(chroma, chroma0)
