"""ff_sharpen on the GPU: bit for bit, radiance and bytes, against the numpy float32 restatement (tests/sharpen_ref.py) and against the
host twin over image sizes around the kernel's 32 x 8 tiles, both instantiations and four strengths; unusable pixels beside the tile
seams; the identities; buffer kinds and refused aliasing; the work buffer regrown; isolation from the other entry points; and the
chain render -> ff_gbuffer -> ff_denoise -> ff_sharpen -> ff_display on a real 1-spp frame."""
import ctypes as C

import numpy as np
import pytest

from gpupathtracer_amd import lib, scenes
from gpupathtracer_amd import types as T
import sharpen_ref as R
from sharpen_cases import BIG, FLAG_SETTINGS, PLANT_SIZE, SEAM_UNUSABLE, SIZES, STRENGTHS, UNUSABLE, assert_same, corners, cross, inputs, reference

pytestmark = pytest.mark.gpu

F = np.float32
C2_POSE = dict(yaw=-90.0, pitch=0.0)


def check_all_three(tracer, rad, p):
    got = tracer.sharpen(rad, p)
    assert_same(got, reference(rad, p))
    assert_same(got, lib.sharpen_host(rad, p))
    return got


@pytest.mark.parametrize("w,h", SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
def test_reference_and_twin_parity_bit_for_bit(tracer, w, h):
    rad = inputs(w, h)
    changed = 0
    for flags in FLAG_SETTINGS:
        for strength in STRENGTHS:
            out = check_all_three(tracer, rad, lib.sharpen_params(strength=strength, flags=flags))[1]
            changed += int((R.bits(out) != R.bits(rad)).sum())
    assert changed or w * h <= 4


def test_parity_at_320x180(tracer):
    rad = inputs(*BIG)
    for flags in FLAG_SETTINGS:
        out = check_all_three(tracer, rad, lib.sharpen_params(strength=1.0, flags=flags))[1]
        assert (R.bits(out) != R.bits(rad)).any(axis=-1).sum() > BIG[0] * BIG[1] // 2


def test_unusable_pixels_beside_the_tile_seams(tracer):
    """The unusable pixels of SEAM_UNUSABLE lie on both sides of x = 31 | 32 and y = 7 | 8 and at the corners (32, 8) and (64, 8) of
    the kernel's tiles: the pixel across the seam is copied through exactly when the apron delivered its unusable neighbour, and the
    diagonal neighbours - the corners the apron leaves out - are sharpened."""
    w, h = PLANT_SIZE
    rad = inputs(w, h)
    for flags in FLAG_SETTINGS:
        out = check_all_three(tracer, rad, lib.sharpen_params(strength=1.0, flags=flags))[1]
        for y, x in list(UNUSABLE) + SEAM_UNUSABLE:
            assert np.array_equal(R.bits(out[y, x]), R.bits(rad[y, x]))
            for q in cross(y, x, w, h):
                assert np.array_equal(R.bits(out[q]), R.bits(rad[q])), ((y, x), q)
            for q in corners(y, x, w, h):
                assert not np.array_equal(R.bits(out[q]), R.bits(rad[q])), ((y, x), q)
    # the same pixels made usable: their neighbours across the seams are sharpened
    clean = np.array(rad)
    for y, x in SEAM_UNUSABLE:
        clean[y, x] = (0.5, 0.4, 0.3)
    out = check_all_three(tracer, clean, lib.sharpen_params(strength=1.0))[1]
    for y, x in SEAM_UNUSABLE:
        for q in cross(y, x, w, h):
            assert not np.array_equal(R.bits(out[q]), R.bits(clean[q])), ((y, x), q)


def test_identities_on_the_device(tracer):
    rad = inputs(*PLANT_SIZE)
    for flags in FLAG_SETTINGS:
        for zero in (0.0, -0.0):
            rgb8, out = check_all_three(tracer, rad, lib.sharpen_params(strength=zero, flags=flags))
            assert np.array_equal(R.bits(out), R.bits(rad)) and np.array_equal(rgb8, R.to_u8(rad))
    flat = np.empty((17, 65, 3), F)
    flat[:] = (0.7, -0.0, 3.0)
    one = np.array([[[0.25, 1.0e5, 0.0]]], F)
    for img in (flat, one, np.zeros((9, 33, 3), F)):
        for flags in FLAG_SETTINGS:
            rgb8, out = check_all_three(tracer, img, lib.sharpen_params(strength=1.0, flags=flags))
            assert np.array_equal(R.bits(out), R.bits(img)) and np.array_equal(rgb8, R.to_u8(img))


def test_buffer_kinds_and_aliasing(tracer):
    import torch
    w, h = PLANT_SIZE
    rad = inputs(w, h)
    p = lib.sharpen_params(strength=0.75)
    host8, host_out = check_all_three(tracer, rad, p)
    # only the bytes, only the floats, neither
    got = tracer.sharpen(rad, p, want_out=False)
    assert got[1] is None and np.array_equal(got[0], host8)
    got = tracer.sharpen(rad, p, want_rgb8=False)
    assert got[0] is None and np.array_equal(R.bits(got[1]), R.bits(host_out))
    assert tracer.sharpen(rad, p, want_rgb8=False, want_out=False) == (None, None)
    # a device tensor through the same method
    d_rad = torch.from_numpy(np.array(rad)).cuda()
    t8, t_out = tracer.sharpen(d_rad, p)
    assert t8.is_cuda and t_out.is_cuda
    assert_same((t8.cpu().numpy(), t_out.cpu().numpy()), (host8, host_out))
    assert np.array_equal(R.bits(d_rad.cpu().numpy()), R.bits(rad))  # (the input is left alone)
    t8, none = tracer.sharpen(d_rad, p, want_out=False)
    assert none is None and np.array_equal(t8.cpu().numpy(), host8)
    # raw pointers: one output at a time, then neither
    d8 = torch.zeros((h, w, 3), dtype=torch.uint8, device="cuda")
    d_out = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    src = d_rad.data_ptr()
    tracer.sharpen_device(w, h, src, p, d8.data_ptr(), None)
    assert np.array_equal(d8.cpu().numpy(), host8)
    tracer.sharpen_device(w, h, src, p, None, d_out.data_ptr())
    assert np.array_equal(R.bits(d_out.cpu().numpy()), R.bits(host_out))
    tracer.sharpen_device(w, h, src, p, None, None)
    # buffers that are only 4-byte (1-byte) aligned
    big = torch.zeros(h * w * 3 + 8, dtype=torch.float32, device="cuda")
    big[1:1 + h * w * 3] = d_rad.reshape(-1)
    big_out = torch.zeros(h * w * 3 + 8, dtype=torch.float32, device="cuda")
    b8 = torch.zeros(h * w * 3 + 8, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    tracer.sharpen_device(w, h, big.data_ptr() + 4, p, b8.data_ptr() + 1, big_out.data_ptr() + 4)
    assert np.array_equal(b8.cpu().numpy()[1:1 + h * w * 3].reshape(h, w, 3), host8)
    assert np.array_equal(R.bits(big_out.cpu().numpy()[1:1 + h * w * 3].reshape(h, w, 3)), R.bits(host_out))
    assert (big_out.cpu().numpy()[[0, -7]] == 0).all() and (b8.cpu().numpy()[[0, -7]] == 0).all()
    # mixed: a device input with host outputs, a host input with device outputs, through the raw entry point
    lib_ = lib.load()
    m8, m_out = np.zeros((h, w, 3), np.uint8), np.zeros((h, w, 3), np.float32)
    vp = C.c_void_p
    lib.check(lib_.ff_sharpen(tracer._state, w, h, C.byref(p), vp(src), 1, m8.ctypes.data, 0, m_out.ctypes.data, 0))
    assert_same((m8, m_out), (host8, host_out))
    d8.zero_()
    d_out.zero_()
    torch.cuda.synchronize()
    lib.check(lib_.ff_sharpen(tracer._state, w, h, C.byref(p), rad.ctypes.data, 0, vp(d8.data_ptr()), 1, vp(d_out.data_ptr()), 1))
    assert_same((d8.cpu().numpy(), d_out.cpu().numpy()), (host8, host_out))
    # an output on the input or on the other output is refused on the host: nothing is launched, nothing is written
    d_out.fill_(7.0)
    torch.cuda.synchronize()
    last = src + 12 * w * h - 4
    for args, words in [((None, src), "radiance_out overlaps radiance_in"), ((None, src + 12), "radiance_out overlaps radiance_in"),
                        ((None, last), "radiance_out overlaps radiance_in"), ((src + 16, None), "rgb8 overlaps radiance_in"),
                        ((d_out.data_ptr() + 64, d_out.data_ptr()), "rgb8 overlaps radiance_out"),
                        ((d_out.data_ptr(), d_out.data_ptr() + 3 * w * h - 1), "rgb8 overlaps radiance_out")]:  # (3 w h - 1 = 20300: by one byte)
        with pytest.raises(lib.FireflyError) as e:
            tracer.sharpen_device(w, h, src, p, *args)
        assert e.value.status == T.FF_ERR_INVALID_ARG and words in e.value.message
    assert (d_out.cpu().numpy() == 7.0).all()
    assert np.array_equal(R.bits(d_rad.cpu().numpy()), R.bits(rad))


def test_the_work_buffer_regrows(tracer):
    p = lib.sharpen_params(strength=1.0)
    for w, h in (BIG, (33, 9), BIG, (1, 1), PLANT_SIZE):
        rad = inputs(w, h)
        assert_same(tracer.sharpen(rad, p), lib.sharpen_host(rad, p))


def test_sharpen_is_not_a_frame(tracer):
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
    assert_same(tracer.sharpen(second[1]), reference(second[1], lib.sharpen_params()))
    tracer.sharpen(inputs(*BIG), lib.sharpen_params(strength=1.0, flags=0))  # (a larger image: the work buffer is regrown)
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


def test_no_scene_is_needed_and_arguments_are_checked_first():
    rad = inputs(17, 15)
    with lib.Tracer(0) as t:
        p = lib.sharpen_params()
        assert_same(t.sharpen(rad, p), lib.sharpen_host(rad, p))
        out = np.full(rad.shape, 7.0, np.float32)
        lib_ = lib.load()
        for field, value in [("strength", 1.5), ("strength", float("nan")), ("flags", 2), ("reserved", 1)]:
            q = lib.sharpen_params(**{field: value})
            assert lib_.ff_sharpen(t._state, 17, 15, C.byref(q), rad.ctypes.data, 0, None, 0, out.ctypes.data, 0) == T.FF_ERR_INVALID_ARG
            assert field in lib_.ff_last_error().decode()
        assert lib_.ff_sharpen(t._state, 17, 15, C.byref(p), None, 0, None, 0, out.ctypes.data, 0) == T.FF_ERR_INVALID_ARG
        assert "radiance_in" in lib_.ff_last_error().decode()
        assert lib_.ff_sharpen(t._state, 0, 15, C.byref(p), rad.ctypes.data, 0, None, 0, out.ctypes.data, 0) == T.FF_ERR_INVALID_ARG
        assert "size" in lib_.ff_last_error().decode()
        assert (out == 7.0).all()


def test_chain_on_a_real_frame(tracer):
    """A 1-spp frame of the mirror Cornell box with next-event estimation, its G-buffer, the denoiser, the sharpening, the display
    transform: the kernel against the twin and the restatement on what ff_denoise really produces."""
    w, h = 64, 36
    tracer.upload_scene(scenes.cornell_mirror_scene())
    cam = scenes.posed_camera(w, h, position=(0.0, 0.0, 5.0), **C2_POSE)  # (from outside the open front: the light and misses are in view)
    gb = tracer.gbuffer(cam, lib.render_params(w, h))
    rad = tracer.render(cam, lib.render_params(w, h, 8, 1, seed=11, shade_mode=T.SHADE_DIFFUSE_PATH_NEE))[1]
    denoised = tracer.denoise(rad, gb)[1]
    for p in (lib.sharpen_params(), lib.sharpen_params(strength=1.0, flags=0)):
        rgb8, out = check_all_three(tracer, denoised, p)
        hit = (R.bits(out) != R.bits(denoised)).any(axis=-1)
        print(f"strength {p.strength} flags {p.flags}: {int(hit.sum())} of {w * h} pixels changed, mean {out.mean():.5g} of {denoised.mean():.5g}")
        assert hit.sum() > w * h // 4 and np.isfinite(out[hit]).all() and (out[hit] >= 0).all()
        shown8, shown = tracer.display(out, lib.display_params())
        assert np.isfinite(shown).all() and shown8.any()
