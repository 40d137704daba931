"""ff_interpolate on the GPU: bit for bit - radiance, bytes and the five counts - against the numpy float32 restatement
(tests/interpolate_ref.py) and against the host twin over image sizes around the kernels' 256-wide rows and 32 x 8 tiles, four t,
four fill radii, with and without geometry maps; holes planted beside the fill kernel's tile seams; buffer kinds and refused
overlap; the work buffer regrown; isolation from the other entry points; and the chain ff_render at two poses -> ff_gbuffer at
three -> ff_interpolate -> ff_display on a real scene."""
import ctypes as C

import numpy as np
import pytest

from gpupathtracer_amd import lib, scenes
from gpupathtracer_amd import types as T
import interpolate_cases as IC
import interpolate_ref as R

pytestmark = pytest.mark.gpu

F = np.float32
C2_POSE = dict(yaw=-90.0, pitch=0.0)


def args_of(c):
    return (c["mid"][0], c["mid"][1:]), (c["a"][0], c["a"][1], c["a"][2:]), (c["b"][0], c["b"][1], c["b"][2:])


def same(got, want):
    assert R.same_bits(got[1], want[1]), np.argwhere((got[1].view(np.uint32) != want[1].view(np.uint32)).any(-1))[:5]
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[2], want[2]), (got[2], want[2])


def check_all_three(tracer, c, **params):
    p = lib.interpolate_params(**params)
    got = tracer.interpolate(*args_of(c), p, c["maps"])
    out, rgb8, counts, state = IC.ref(c, **params)
    same(got, (rgb8, out, counts))
    same(got, lib.interpolate_host(*args_of(c), p, c["maps"]))
    return got, state


@pytest.mark.parametrize("size", IC.SIZES + [IC.MAIN], ids=lambda s: f"{s[0]}x{s[1]}")
def test_reference_and_twin_parity_bit_for_bit(tracer, size):
    for moving in (False, True):
        c = IC.case(size, moving)
        for t in IC.TS:
            check_all_three(tracer, c, t=t)
        for r in IC.RADII:
            check_all_three(tracer, c, t=0.25, fill_radius=r)


def test_parity_at_320x180(tracer):
    for moving in (False, True):
        got, state = check_all_three(tracer, IC.case(IC.LARGE, moving))
        assert (got[2] > 0).all() and got[2].sum() == IC.LARGE[0] * IC.LARGE[1], got[2]


def test_seam_holes_and_planted_non_finite_pixels(tracer):
    c, hole = IC.seam_holes()
    for r in IC.RADII:
        got, state = check_all_three(tracer, c, fill_radius=r)
        assert np.array_equal(state >= R.FILLED, hole) and got[2][R.FILLED:].sum() == hole.sum()
    planted = IC.planted_nonfinite(IC.case(IC.MAIN, True))
    got, state = check_all_three(tracer, planted, t=0.25)
    assert np.isfinite(got[1][state != R.FALLBACK]).all()


def device_call(tracer, c, p, rgb8=True, out=True, on=None):
    """ff_interpolate on device tensors -> (rgb8, radiance, counts) as host arrays (None where not asked for)."""
    import torch
    (cm, pm, im), (ca, ra, pa, ia), (cb, rb, pb, ib) = c["mid"], c["a"], c["b"]
    h, w = im.shape[:2]
    dev = [torch.from_numpy(np.array(x)).cuda() for x in (pm, im, ra, pa, ia, rb, pb, ib)]
    d8 = torch.zeros((h, w, 3), dtype=torch.uint8, device="cuda") if rgb8 else None
    d_out = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda") if out else None
    torch.cuda.synchronize()
    counts = tracer.interpolate_device(w, h, (cm, ca, cb), [x.data_ptr() for x in dev], p, c["maps"], d8.data_ptr() if rgb8 else None,
                                       d_out.data_ptr() if out else None)
    for x, host in zip(dev, (pm, im, ra, pa, ia, rb, pb, ib)):  # (the inputs are left alone)
        assert x.cpu().numpy().tobytes() == np.ascontiguousarray(host).tobytes()
    return (d8.cpu().numpy() if rgb8 else None, d_out.cpu().numpy() if out else None, counts), dev


def test_buffer_kinds_and_refused_overlap(tracer):
    import torch
    c = IC.case((65, 17), True)
    p = lib.interpolate_params(t=0.25)
    host = tracer.interpolate(*args_of(c), p, c["maps"])
    same(host, lib.interpolate_host(*args_of(c), p, c["maps"]))
    got = tracer.interpolate(*args_of(c), p, c["maps"], want_out=False)
    assert got[1] is None and np.array_equal(got[0], host[0]) and np.array_equal(got[2], host[2])
    got = tracer.interpolate(*args_of(c), p, c["maps"], want_rgb8=False)
    assert got[0] is None and R.same_bits(got[1], host[1])
    got, dev = device_call(tracer, c, p)
    same(got, host)
    got, _ = device_call(tracer, c, p, rgb8=False)
    assert got[0] is None and R.same_bits(got[1], host[1]) and np.array_equal(got[2], host[2])
    got, _ = device_call(tracer, c, p, out=False)
    assert got[1] is None and np.array_equal(got[0], host[0])
    # device inputs with host outputs through the raw entry point
    w, h = 65, 17
    m8, m_out, counts = np.zeros((h, w, 3), np.uint8), np.zeros((h, w, 3), F), np.zeros(5, np.uint32)
    vp = C.c_void_p
    d = [vp(x.data_ptr()) for x in dev]
    cams = [C.byref(c[k][0]) for k in ("mid", "a", "b")]
    maps = np.ascontiguousarray(c["maps"], F)
    call = lambda rgb8, rgb8_dev, out, out_dev: lib.load().ff_interpolate(  # noqa: E731
        tracer._state, w, h, C.byref(p), cams[0], d[0], d[1], cams[1], d[2], d[3], d[4], cams[2], d[5], d[6], d[7], maps.ctypes.data, maps.shape[0], 1,
        rgb8, rgb8_dev, out, out_dev, counts.ctypes.data)
    lib.check(call(m8.ctypes.data, 0, m_out.ctypes.data, 0))
    same((m8, m_out, counts), host)
    # an output on an input or on the other output is refused on the host: nothing is launched, nothing is written
    d_out = torch.full((h, w, 3), 7.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    names = ("position", "ids", "radiance_a", "position_a", "ids_a", "radiance_b", "position_b", "ids_b")
    last = lambda: lib.load().ff_last_error().decode()  # noqa: E731
    for x, name in zip(dev, names):
        assert call(None, 1, vp(x.data_ptr()), 1) == T.FF_ERR_INVALID_ARG and f"radiance_out overlaps {name}" in last(), (name, last())
        assert call(vp(x.data_ptr() + 9 * w * h), 1, vp(d_out.data_ptr()), 1) == T.FF_ERR_INVALID_ARG and f"rgb8 overlaps {name}" in last()
    assert call(vp(d_out.data_ptr() + 64), 1, vp(d_out.data_ptr()), 1) == T.FF_ERR_INVALID_ARG and "rgb8 overlaps radiance_out" in last()
    assert (d_out.cpu().numpy() == 7.0).all()


def test_the_work_buffer_regrows(tracer):
    for size in ((33, 9), IC.LARGE, (1, 1), IC.MAIN, IC.LARGE):
        c = IC.case(size, size == IC.MAIN)
        p = lib.interpolate_params(t=0.25)
        same(tracer.interpolate(*args_of(c), p, c["maps"]), lib.interpolate_host(*args_of(c), p, c["maps"]))


def test_interpolate_is_not_a_frame(tracer):
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
    taa_hist, tp_hist = tracer.taa_history(), tracer.temporal_history()

    def snapshot():
        s = tracer.stats()
        return {f: getattr(s, f) for f, _ in s._fields_}
    before = snapshot()
    c = IC.case(IC.MAIN)
    tracer.interpolate(*args_of(c))
    big = IC.case(IC.LARGE)
    tracer.interpolate(*args_of(big))          # (a larger image: the work buffer is regrown)
    assert snapshot() == before and tracer.kernel_name() == name
    for a, b in zip(tracer.taa_history() + tracer.temporal_history(), taa_hist + tp_hist):
        assert np.array_equal(np.asarray(a).view(np.uint32), np.asarray(b).view(np.uint32))
    again = tracer.gbuffer(cam, flat)          # (at rest: the stored primary hits are still there and still this frame's)
    for key in gb:
        assert np.array_equal(np.asarray(again[key]).view(np.uint32), np.asarray(gb[key]).view(np.uint32)), key
    third = tracer.render(cam, prm)
    assert np.array_equal(third[0], second[0]) and R.same_bits(third[1], second[1]) and R.same_bits(first[1], second[1])
    s3 = tracer.stats()
    assert (s3.rays_answered, s3.rays_traced, s3.flags, s3.kernel_launches) == (st.rays_answered, st.rays_traced, st.flags, st.kernel_launches)


def test_no_scene_is_needed_and_arguments_are_checked_first():
    c = IC.case((33, 9))
    with lib.Tracer(0) as t:
        same(t.interpolate(*args_of(c)), lib.interpolate_host(*args_of(c)))
        for field, value in [("t", 1.5), ("t", float("nan")), ("surface_tolerance", 0.0), ("fill_radius", 9), ("flags", 1), ("reserved", 1)]:
            with pytest.raises(lib.FireflyError) as e:
                t.interpolate(*args_of(c), lib.interpolate_params(**{field: value}))
            assert e.value.status == T.FF_ERR_INVALID_ARG and field in e.value.message


def test_chain_on_a_real_scene(tracer):
    """ff_render at two poses of the Cornell box with spheres, ff_gbuffer at three, ff_interpolate for the pose between, ff_display:
    the kernels against the twin and the restatement on what the tracer really produces, and the in-between frame against the
    plain blend of its neighbours."""
    w, h = 64, 36
    tracer.upload_scene(scenes.cornell_spheres_scene())
    cams = [scenes.posed_camera(w, h, position=(x, 0.0, 2.4), **C2_POSE) for x in (-0.35, 0.0, 0.35)]
    flat = lib.render_params(w, h)
    gbs = [tracer.gbuffer(cam, flat) for cam in cams]
    prm = lib.render_params(w, h, 1, 1, shade_mode=T.SHADE_NORMAL_DEBUG)
    ra, truth, rb = (tracer.render(cam, prm)[1] for cam in cams)
    c = {"mid": (cams[1], gbs[1]["position"], gbs[1]["ids"]), "a": (cams[0], ra, gbs[0]["position"], gbs[0]["ids"]),
         "b": (cams[2], rb, gbs[2]["position"], gbs[2]["ids"]), "maps": None}
    (rgb8, out, counts), state = check_all_three(tracer, c)
    mse = ((out.astype(np.float64) - truth) ** 2).mean()
    blend = (((ra.astype(np.float64) + rb) / 2 - truth) ** 2).mean()
    print(f"counts {counts.tolist()}, interpolated MSE {mse:.6g}, blend MSE {blend:.6g}")
    assert counts[R.BOTH] > w * h // 2 and counts[R.A_ONLY] and counts[R.B_ONLY] and mse < blend
    shown8, shown = tracer.display(out, lib.display_params())
    assert np.isfinite(shown).all() and shown8.any()
