"""ff_motion_blur on the GPU: bit for bit against the numpy float32 reference (tests/motion_blur_ref.py) and against the host twin
over image sizes, tile edges, tap counts and shutters; the identities; buffer kinds and refused aliasing; the pipeline
render -> ff_gbuffer -> ff_taa -> ff_motion_blur under a sliding camera and at rest; isolation from the other entry points."""
import ctypes as C

import numpy as np
import pytest

from gpupathtracer_amd import lib, scenes
from gpupathtracer_amd import types as T
import motion_blur_ref as R
from motion_blur_cases import SIZES, assert_same, inputs, params_of

pytestmark = pytest.mark.gpu

F = np.float32
C2_POSE = dict(yaw=-90.0, pitch=0.0)
# (max_radius, samples, shutter): thinner than the host test's grid, every value of each axis present
PARAMS = [(16, 15, 0.5), (1, 1, 4.0), (2, 64, 1.0), (64, 2, 0.25), (16, 15, 4.0), (64, 64, 1.0)]
# tiles of up to 8 x 8 pixels are packed by lane groups of 1, 4, 16, 32 and 64 lanes: every group size with idle lanes, and both
# sides of the edge to one workgroup per tile
SMALL_TILES = [(3, 15, 1.0), (4, 15, 1.0), (5, 15, 1.0), (7, 15, 2.0), (8, 15, 1.0), (9, 15, 1.0)]


def check_all_three(tracer, rad, motion, depth, p):
    got = tracer.motion_blur(rad, motion, depth, p)
    assert_same(got, R.motion_blur(rad, motion, depth, **params_of(p)))
    assert_same(got, lib.motion_blur_host(rad, motion, depth, p))
    return got


@pytest.mark.parametrize("w,h", SIZES + [(320, 180)], ids=[f"{w}x{h}" for w, h in SIZES + [(320, 180)]])
def test_reference_and_twin_parity_bit_for_bit(tracer, w, h):
    rad, motion, depth = inputs(w, h)
    blurred = 0
    for k, S, shutter in (PARAMS if w * h < 320 * 180 else PARAMS[:3]):
        out = check_all_three(tracer, rad, motion, depth, lib.motion_blur_params(shutter=shutter, max_radius=k, samples=S))[1]
        blurred += int((R.bits(out) != R.bits(rad)).any())
    assert blurred or w * h == 1


@pytest.mark.parametrize("w,h", [(33, 31), (101, 67), (320, 180)], ids=["33x31", "101x67", "320x180"])
def test_small_tiles_bit_for_bit(tracer, w, h):
    rad, motion, depth = inputs(w, h)
    for k, S, shutter in SMALL_TILES:
        check_all_three(tracer, rad, motion, depth, lib.motion_blur_params(shutter=shutter, max_radius=k, samples=S))


def test_identities_on_the_device(tracer):
    w, h = 33, 31
    rad, motion, depth = inputs(w, h)
    dirty = rad.copy()
    dirty[3, 4] = (np.nan, 0.5, 0.25)
    dirty[10, 20] = np.inf
    dirty[30, 32] = (-np.inf, np.nan, 1.0)
    flat = np.empty_like(rad)
    flat[:] = (0.7, 0.05, 3.0)
    for p in (lib.motion_blur_params(), lib.motion_blur_params(shutter=4.0, max_radius=2, samples=64)):
        p0 = lib.motion_blur_params(**dict(params_of(p), shutter=0.0))
        p1 = lib.motion_blur_params(**dict(params_of(p), shutter=1.0))
        for image, m, q in [(rad, np.zeros_like(motion), p), (dirty, np.zeros_like(motion), p), (rad, motion, p0), (dirty, motion, p0), (flat, motion, p1)]:
            rgb8, out = tracer.motion_blur(image, m, depth, q)
            assert np.array_equal(R.bits(out), R.bits(image)) and np.array_equal(rgb8, R.to_u8(image))
    # a -0 channel of a constant colour stays -0
    flat[..., 1] = -0.0
    rgb8, out = check_all_three(tracer, flat, motion, depth, lib.motion_blur_params(shutter=1.0))
    assert np.array_equal(R.bits(out), R.bits(flat))
    # a non-finite pixel under moving neighbours spoils only itself
    moving = np.broadcast_to(np.array([14.0, 5.0], np.float32), motion.shape)
    rgb8, out = check_all_three(tracer, dirty, moving, depth, lib.motion_blur_params(shutter=1.0))
    bad = ~np.isfinite(dirty).all(axis=-1)
    assert np.isfinite(out[~bad]).all() and np.array_equal(R.bits(out[bad]), R.bits(dirty[bad]))


def test_buffer_kinds_and_aliasing(tracer):
    import torch
    w, h = 101, 67
    rad, motion, depth = inputs(w, h)
    p = lib.motion_blur_params(shutter=1.0)
    host8, host_out = check_all_three(tracer, rad, motion, depth, p)
    # only the bytes, only the floats, neither
    assert np.array_equal(tracer.motion_blur(rad, motion, depth, p, want_out=False)[0], host8)
    assert np.array_equal(R.bits(tracer.motion_blur(rad, motion, depth, p, want_rgb8=False)[1]), R.bits(host_out))
    assert tracer.motion_blur(rad, motion, depth, p, want_rgb8=False, want_out=False) == (None, None)
    # device buffers
    d_rad, d_motion, d_depth = (torch.from_numpy(np.array(a)).cuda() for a in (rad, motion, depth))
    d8 = torch.zeros((h, w, 3), dtype=torch.uint8, device="cuda")
    d_out = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    tracer.motion_blur_device(w, h, d_rad.data_ptr(), d_motion.data_ptr(), d_depth.data_ptr(), p, d8.data_ptr(), d_out.data_ptr())
    assert np.array_equal(d8.cpu().numpy(), host8) and np.array_equal(R.bits(d_out.cpu().numpy()), R.bits(host_out))
    for d, a in ((d_rad, rad), (d_motion, motion), (d_depth, depth)):
        assert np.array_equal(R.bits(d.cpu().numpy()), R.bits(a))  # (the inputs are left alone)
    d8.zero_()
    tracer.motion_blur_device(w, h, d_rad.data_ptr(), d_motion.data_ptr(), d_depth.data_ptr(), p, d8.data_ptr(), None)
    assert np.array_equal(d8.cpu().numpy(), host8)
    d_out.zero_()
    tracer.motion_blur_device(w, h, d_rad.data_ptr(), d_motion.data_ptr(), d_depth.data_ptr(), p, None, d_out.data_ptr())
    assert np.array_equal(R.bits(d_out.cpu().numpy()), R.bits(host_out))
    # buffers that are only 4-byte aligned
    big = torch.zeros(h * w * 6 + 8, dtype=torch.float32, device="cuda")
    big[1:1 + h * w * 3] = d_rad.reshape(-1)
    big[h * w * 3 + 4:h * w * 5 + 4] = d_motion.reshape(-1)
    b8 = torch.zeros(h * w * 3 + 8, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    tracer.motion_blur_device(w, h, big.data_ptr() + 4, big.data_ptr() + 4 * (h * w * 3 + 4), d_depth.data_ptr(), p, b8.data_ptr() + 1, d_out.data_ptr())
    assert np.array_equal(b8.cpu().numpy()[1:1 + h * w * 3].reshape(h, w, 3), host8) and np.array_equal(R.bits(d_out.cpu().numpy()), R.bits(host_out))
    # mixed: device inputs with host outputs, host inputs with device outputs, through the raw entry point
    lib_ = lib.load()
    m8, m_out = np.zeros((h, w, 3), np.uint8), np.zeros((h, w, 3), np.float32)
    vp = C.c_void_p
    lib.check(lib_.ff_motion_blur(tracer._state, w, h, C.byref(p), vp(d_rad.data_ptr()), vp(d_motion.data_ptr()), vp(d_depth.data_ptr()), 1,
                                  m8.ctypes.data, 0, m_out.ctypes.data, 0))
    assert np.array_equal(m8, host8) and np.array_equal(R.bits(m_out), R.bits(host_out))
    d8.zero_()
    d_out.zero_()
    torch.cuda.synchronize()
    lib.check(lib_.ff_motion_blur(tracer._state, w, h, C.byref(p), rad.ctypes.data, motion.ctypes.data, depth.ctypes.data, 0, vp(d8.data_ptr()), 1,
                                  vp(d_out.data_ptr()), 1))
    assert np.array_equal(d8.cpu().numpy(), host8) and np.array_equal(R.bits(d_out.cpu().numpy()), R.bits(host_out))
    # an output on an input is refused and nothing is written
    with pytest.raises(lib.FireflyError) as e:
        tracer.motion_blur_device(w, h, d_rad.data_ptr(), d_motion.data_ptr(), d_depth.data_ptr(), p, None, d_rad.data_ptr())
    assert e.value.status == T.FF_ERR_INVALID_ARG and "radiance_out overlaps radiance_in" in e.value.message
    with pytest.raises(lib.FireflyError) as e:
        tracer.motion_blur_device(w, h, d_rad.data_ptr(), d_motion.data_ptr(), d_depth.data_ptr(), p, d_motion.data_ptr() + 16, None)
    assert e.value.status == T.FF_ERR_INVALID_ARG and "rgb8 overlaps motion" in e.value.message
    with pytest.raises(lib.FireflyError) as e:
        tracer.motion_blur_device(w, h, d_rad.data_ptr(), d_motion.data_ptr(), d_depth.data_ptr(), p, d_out.data_ptr() + 64, d_out.data_ptr())
    assert e.value.status == T.FF_ERR_INVALID_ARG and "rgb8 overlaps radiance_out" in e.value.message
    assert np.array_equal(R.bits(d_rad.cpu().numpy()), R.bits(rad)) and np.array_equal(R.bits(d_motion.cpu().numpy()), R.bits(motion))


def test_pipeline_under_a_sliding_camera_and_at_rest(tracer):
    w, h = 64, 48
    tracer.upload_scene(scenes.cornell_wahoo_scene())
    tracer.taa_reset()
    flat = lib.render_params(w, h)
    cams = [scenes.posed_camera(w, h, position=(x, 0.0, 2.4), **C2_POSE) for x in (0.0, 0.25, 0.25)]
    p = lib.motion_blur_params(shutter=1.0)
    results = []
    for i, cam in enumerate(cams):
        gb = tracer.gbuffer(cam, flat)
        rad = tracer.render(cam, lib.render_params(w, h, 6, 1, 40 + i))[1]
        resolved = tracer.taa(rad, gb, cam)[1]
        motion = tracer.taa_history()[0]
        results.append((resolved, motion, check_all_three(tracer, resolved, motion, gb["depth"], p)))
    resolved, motion, (rgb8, out) = results[1]
    assert np.abs(motion).max() > 1.0  # the camera slid: there is something to blur along
    assert (R.bits(out) != R.bits(resolved)).any() and np.isfinite(out).all()
    resolved, motion, (rgb8, out) = results[2]  # the camera bitwise at rest
    assert not motion.any()
    assert np.array_equal(R.bits(out), R.bits(resolved)) and np.array_equal(rgb8, R.to_u8(resolved))


def test_motion_blur_is_not_a_frame(tracer):
    w, h = 96, 64
    scene = scenes.cornell_wahoo_scene()
    cam = scenes.posed_camera(w, h, position=(0.0, 0.0, 2.4), **C2_POSE)
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
    tracer.display(second[1], lib.display_params(flags=T.DISPLAY_AUTO_EXPOSURE))
    taa_hist, tp_hist, disp = tracer.taa_history(), tracer.temporal_history(), tracer.display_state()

    def snapshot():
        s = tracer.stats()
        return {f: getattr(s, f) for f, _ in s._fields_}
    before = snapshot()
    rad, motion, depth = inputs(w, h)
    tracer.motion_blur(second[1], motion, gb["depth"], lib.motion_blur_params(shutter=1.0))
    big = inputs(640, 360)                      # (a larger image: the work buffer is regrown)
    tracer.motion_blur(*big, lib.motion_blur_params(max_radius=64))
    assert_same(tracer.motion_blur(rad, motion, depth), lib.motion_blur_host(rad, motion, depth))  # (... and a smaller one again)
    assert snapshot() == before
    for a, b in zip(tracer.taa_history() + tracer.temporal_history(), taa_hist + tp_hist):
        assert np.array_equal(R.bits(a), R.bits(b))
    after = tracer.display_state()
    assert after[:2] == disp[:2] and np.array_equal(after[2], disp[2])
    third = tracer.render(cam, prm)
    assert np.array_equal(third[0], second[0]) and np.array_equal(R.bits(third[1]), R.bits(second[1]))
    assert np.array_equal(R.bits(first[1]), R.bits(second[1]))
    s3 = tracer.stats()
    assert (s3.rays_answered, s3.rays_traced, s3.flags, s3.kernel_launches) == (st.rays_answered, st.rays_traced, st.flags, st.kernel_launches)


def test_no_scene_is_needed_and_arguments_are_checked_first():
    rad, motion, depth = inputs(17, 9)
    with lib.Tracer(0) as t:
        assert_same(t.motion_blur(rad, motion, depth), lib.motion_blur_host(rad, motion, depth))
        out = np.full(rad.shape, 7.0, np.float32)
        lib_ = lib.load()
        for field, value in [("shutter", 5.0), ("max_radius", 0), ("samples", 65), ("depth_extent", 0.0), ("flags", 2), ("reserved", 1)]:
            p = lib.motion_blur_params(**{field: value})
            assert lib_.ff_motion_blur(t._state, 17, 9, C.byref(p), rad.ctypes.data, motion.ctypes.data, depth.ctypes.data, 0, None, 0, out.ctypes.data,
                                       0) == T.FF_ERR_INVALID_ARG
            assert field in lib_.ff_last_error().decode()
        assert (out == 7.0).all()
