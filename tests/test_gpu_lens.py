"""ff_lens on the GPU: bit for bit, radiance and bytes, against the numpy float32 restatement (tests/lens_ref.py) and against the host
twin over image sizes around the kernel's 32 x 8 tiles and parameter sets that reach all six instantiations; non-finite pixels beside
the tile seams; buffer kinds and refused aliasing; the work buffer regrown and the table's cache; isolation from the other entry
points; and the chain render -> ff_gbuffer -> ff_denoise -> ff_lens -> ff_display on a real 1-spp frame."""
import ctypes as C

import numpy as np
import pytest

from gpupathtracer_amd import lib, scenes
from gpupathtracer_amd import types as T
import lens_ref as R
from lens_cases import BIG, PARAMETER_SETS, PLANT_SIZE, PLANTED, SIZES, assert_same, geometry_on, inputs, instantiation, params, reference

pytestmark = pytest.mark.gpu

F = np.float32
C2_POSE = dict(yaw=-90.0, pitch=0.0)
NAMES = list(PARAMETER_SETS)


def check_all_three(tracer, rad, p):
    got = tracer.lens(rad, p)
    assert_same(got, reference(rad, p))
    assert_same(got, lib.lens_host(rad, p))
    return got


@pytest.mark.parametrize("w,h", SIZES + [BIG], ids=[f"{w}x{h}" for w, h in SIZES + [BIG]])
def test_reference_and_twin_parity_bit_for_bit(tracer, w, h):
    rad = inputs(w, h)
    reached = set()
    for name in NAMES:
        p = params(name)
        out = check_all_three(tracer, rad, p)[1]
        reached.add(instantiation(p))
        if geometry_on(p) and w * h >= 31 * 7:
            assert (R.bits(out) != R.bits(rad)).any(), name  # (the geometry is on: the output is no copy)
    assert reached == {(f, c) for f in (0, 1, 2) for c in (False, True)}
    # the identity, through every filter form and border
    clean = inputs(w, h, planted=False)
    for filt, flags in ((T.LENS_BILINEAR, 0), (T.LENS_CATMULL_ROM, 0), (T.LENS_CATMULL_ROM, T.LENS_ANTI_RING)):
        for border in (T.LENS_BORDER_BLACK, T.LENS_BORDER_CLAMP):
            rgb8, out = check_all_three(tracer, clean, lib.lens_params(filter=filt, flags=flags, border=border))
            assert np.array_equal(R.bits(out), R.bits(clean)) and np.array_equal(rgb8, R.to_u8(clean))


def test_non_finite_pixels_beside_the_tile_seams(tracer):
    """PLANTED puts NaN, +Inf, -Inf and negative pixels on both sides of x = 31 | 32 and y = 7 | 8.  A non-finite tap reads as 0: the
    output is finite, equals the output of the image with those values replaced by 0 bit for bit, and differs from the output of
    the image with them replaced by 7 only where, per the restatement, a tap of that channel read one."""
    w, h = PLANT_SIZE
    rad = inputs(w, h)
    assert {x for (y, x) in PLANTED} >= {31, 32} and {y for (y, x) in PLANTED} >= {7, 8}
    bad = ~np.isfinite(rad)
    zeroed, sevens = np.where(bad, F(0.0), rad), np.where(bad, F(7.0), rad)
    for name in NAMES:
        p = params(name)
        rgb8, out = check_all_three(tracer, rad, p)
        assert np.isfinite(out).all()
        assert_same((rgb8, out), tracer.lens(zeroed, p))
        reads = reference(rad, p, details=True)[2]["reads_nonfinite"]
        other = check_all_three(tracer, sevens, p)[1]
        differs = R.bits(out) != R.bits(other)
        assert differs.any() and not (differs & ~reads).any(), name
        # on both sides of each seam
        ys, xs = np.nonzero(differs.any(axis=-1))
        assert (xs <= 31).any() and (xs >= 32).any() and (ys <= 7).any() and (ys >= 8).any(), name


def test_buffer_kinds_and_aliasing(tracer):
    import torch
    w, h = PLANT_SIZE
    rad = inputs(w, h)
    p = params("pincushion_distort_cr_ring_ca")
    host8, host_out = check_all_three(tracer, rad, p)
    got = tracer.lens(rad, p, want_out=False)
    assert got[1] is None and np.array_equal(got[0], host8)
    got = tracer.lens(rad, p, want_rgb8=False)
    assert got[0] is None and np.array_equal(R.bits(got[1]), R.bits(host_out))
    assert tracer.lens(rad, p, want_rgb8=False, want_out=False) == (None, None)
    # a device tensor through the same method
    d_rad = torch.from_numpy(np.array(rad)).cuda()
    t8, t_out = tracer.lens(d_rad, p)
    assert t8.is_cuda and t_out.is_cuda
    assert_same((t8.cpu().numpy(), t_out.cpu().numpy()), (host8, host_out))
    assert np.array_equal(R.bits(d_rad.cpu().numpy()), R.bits(rad))  # (the input is left alone)
    # raw pointers: one output at a time, then neither
    d8 = torch.zeros((h, w, 3), dtype=torch.uint8, device="cuda")
    d_out = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    src = d_rad.data_ptr()
    tracer.lens_device(w, h, src, p, d8.data_ptr(), None)
    assert np.array_equal(d8.cpu().numpy(), host8)
    tracer.lens_device(w, h, src, p, None, d_out.data_ptr())
    assert np.array_equal(R.bits(d_out.cpu().numpy()), R.bits(host_out))
    tracer.lens_device(w, h, src, p, None, None)
    # buffers that are only 4-byte (1-byte) aligned
    n = h * w * 3
    big = torch.zeros(n + 8, dtype=torch.float32, device="cuda")
    big[1:1 + n] = d_rad.reshape(-1)
    big_out = torch.zeros(n + 8, dtype=torch.float32, device="cuda")
    b8 = torch.zeros(n + 8, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    tracer.lens_device(w, h, big.data_ptr() + 4, p, b8.data_ptr() + 1, big_out.data_ptr() + 4)
    assert np.array_equal(b8.cpu().numpy()[1:1 + n].reshape(h, w, 3), host8)
    assert np.array_equal(R.bits(big_out.cpu().numpy()[1:1 + n].reshape(h, w, 3)), R.bits(host_out))
    assert (big_out.cpu().numpy()[[0, -7]] == 0).all() and (b8.cpu().numpy()[[0, -7]] == 0).all()
    # mixed: a device input with host outputs, a host input with device outputs, through the raw entry point
    lib_ = lib.load()
    m8, m_out = np.zeros((h, w, 3), np.uint8), np.zeros((h, w, 3), np.float32)
    vp = C.c_void_p
    lib.check(lib_.ff_lens(tracer._state, w, h, C.byref(p), vp(src), 1, m8.ctypes.data, 0, m_out.ctypes.data, 0))
    assert_same((m8, m_out), (host8, host_out))
    d8.zero_()
    d_out.zero_()
    torch.cuda.synchronize()
    lib.check(lib_.ff_lens(tracer._state, w, h, C.byref(p), rad.ctypes.data, 0, vp(d8.data_ptr()), 1, vp(d_out.data_ptr()), 1))
    assert_same((d8.cpu().numpy(), d_out.cpu().numpy()), (host8, host_out))
    # the six overlap refusals, on the host: nothing is launched, nothing is written
    d_out.fill_(7.0)
    torch.cuda.synchronize()
    last = src + 12 * w * h - 4
    for args, words in [((None, src), "radiance_out overlaps radiance_in"), ((None, src + 12), "radiance_out overlaps radiance_in"),
                        ((None, last), "radiance_out overlaps radiance_in"), ((src + 16, None), "rgb8 overlaps radiance_in"),
                        ((d_out.data_ptr() + 64, d_out.data_ptr()), "rgb8 overlaps radiance_out"),
                        ((d_out.data_ptr(), d_out.data_ptr() + 3 * w * h - 1), "rgb8 overlaps radiance_out")]:
        with pytest.raises(lib.FireflyError) as e:
            tracer.lens_device(w, h, src, p, *args)
        assert e.value.status == T.FF_ERR_INVALID_ARG and words in e.value.message
    assert (d_out.cpu().numpy() == 7.0).all()
    assert np.array_equal(R.bits(d_rad.cpu().numpy()), R.bits(rad))


def test_the_work_buffer_regrows_and_the_table_is_cached(tracer):
    a, b = params("barrel_undistort_cr_ring"), params("k2_k3_undistort_cr_ca_vignette")
    for w, h in (BIG, (33, 9), BIG, (1, 1), PLANT_SIZE):
        rad = inputs(w, h)
        assert_same(tracer.lens(rad, a), lib.lens_host(rad, a))
    rad = inputs(*PLANT_SIZE)
    tracer.lens(rad, a)
    n = tracer.lens_table_builds()
    tracer.lens(rad, a)
    tracer.lens(rad, params("barrel_undistort_cr_ring", ca_red=0.01, filter=T.LENS_BILINEAR, border=T.LENS_BORDER_CLAMP, flags=0))  # (none feeds the table)
    assert tracer.lens_table_builds() == n
    steps = [params("barrel_undistort_cr_ring", k1=-0.11), params("barrel_undistort_cr_ring", zoom=1.01), params("barrel_undistort_cr_ring", vignette=0.1),
             params("barrel_undistort_cr_ring", direction=T.LENS_DISTORT), params("barrel_undistort_cr_ring", center_y=0.5)]
    for i, q in enumerate(steps):
        assert_same(tracer.lens(rad, q), lib.lens_host(rad, q))
        assert tracer.lens_table_builds() == n + 1 + i
    small = inputs(33, 9)
    tracer.lens(small, steps[-1])  # (the size is part of the key)
    assert tracer.lens_table_builds() == n + len(steps) + 1
    # an upload leaves the table alone
    tracer.upload_scene(scenes.cornell_mirror_scene())
    tracer.lens(small, steps[-1])
    assert tracer.lens_table_builds() == n + len(steps) + 1
    # two parameter sets alternated give the bits of fresh tracers
    with lib.Tracer(0) as fresh_a, lib.Tracer(0) as fresh_b:
        want_a, want_b = fresh_a.lens(rad, a), fresh_b.lens(rad, b)
    for _ in range(2):
        assert_same(tracer.lens(rad, a), want_a)
        assert_same(tracer.lens(rad, b), want_b)


def test_lens_is_not_a_frame(tracer):
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
    p = params("pincushion_distort_cr_ring_ca")
    assert_same(tracer.lens(second[1], p), reference(second[1], p))
    tracer.lens(inputs(*BIG), params("barrel_distort_bilinear"))  # (a larger image: the work buffer is regrown, the table rebuilt)
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
        p = params("k2_k3_offcentre_zoom_bilinear_ca")
        assert_same(t.lens(rad, p), lib.lens_host(rad, p))
        n = t.lens_table_builds()
        out = np.full(rad.shape, 7.0, np.float32)
        lib_ = lib.load()
        for field, value in [("k1", 11.0), ("zoom", float("nan")), ("center_x", 9.0), ("ca_blue", 1.0), ("vignette", 2.0), ("direction", 2), ("filter", 5),
                             ("border", 3), ("flags", 2), ("reserved", 1)]:
            q = lib.lens_params(**{field: value})
            assert lib_.ff_lens(t._state, 17, 15, C.byref(q), rad.ctypes.data, 0, None, 0, out.ctypes.data, 0) == T.FF_ERR_INVALID_ARG
            assert field in lib_.ff_last_error().decode()
        q = lib.lens_params(k1=-0.5)
        assert lib_.ff_lens(t._state, 17, 15, C.byref(q), rad.ctypes.data, 0, None, 0, out.ctypes.data, 0) == T.FF_ERR_INVALID_ARG
        assert "radius" in lib_.ff_last_error().decode()
        assert lib_.ff_lens(t._state, 17, 15, C.byref(p), None, 0, None, 0, out.ctypes.data, 0) == T.FF_ERR_INVALID_ARG
        assert "radiance_in" in lib_.ff_last_error().decode()
        assert lib_.ff_lens(t._state, 0, 15, C.byref(p), rad.ctypes.data, 0, None, 0, out.ctypes.data, 0) == T.FF_ERR_INVALID_ARG
        assert "size" in lib_.ff_last_error().decode()
        assert (out == 7.0).all() and t.lens_table_builds() == n


def test_chain_on_a_real_frame(tracer):
    """A 1-spp frame of the mirror Cornell box with next-event estimation, its G-buffer, the denoiser, the lens - barrel, DISTORT,
    chromatic aberration, vignette, the FILL zoom -, the display transform: the kernel against the twin and the restatement on what
    ff_denoise really produces."""
    w, h = 64, 36
    tracer.upload_scene(scenes.cornell_mirror_scene())
    cam = scenes.posed_camera(w, h, position=(0.0, 0.0, 5.0), **C2_POSE)  # (from outside the open front: the light and misses are in view)
    gb = tracer.gbuffer(cam, lib.render_params(w, h))
    rad = tracer.render(cam, lib.render_params(w, h, 8, 1, seed=11, shade_mode=T.SHADE_DIFFUSE_PATH_NEE))[1]
    denoised = tracer.denoise(rad, gb)[1]
    fields = dict(k1=-0.15, k2=0.02, direction=T.LENS_DISTORT, ca_red=0.004, ca_blue=-0.004, vignette=0.7, vignette_falloff=1.0)
    fill = lib.lens_fit_zoom(w, h, lib.lens_params(**fields), T.LENS_FIT_FILL)
    for more in (dict(), dict(filter=T.LENS_BILINEAR, flags=0)):
        p = lib.lens_params(zoom=fill, **fields, **more)
        rgb8, out = check_all_three(tracer, denoised, p)
        hit = (R.bits(out) != R.bits(denoised)).any(axis=-1)
        print(f"zoom {fill:.5f} filter {p.filter}: {int(hit.sum())} of {w * h} pixels changed, mean {out.mean():.5g} of {denoised.mean():.5g}")
        assert hit.sum() > w * h // 2 and np.isfinite(out).all() and (out >= 0).all()
        shown8, shown = tracer.display(out, lib.display_params())
        assert np.isfinite(shown).all() and shown8.any()
