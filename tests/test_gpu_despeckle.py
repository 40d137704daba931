"""ff_despeckle on the GPU: bit for bit, the count included, against the numpy float32 reference (tests/despeckle_ref.py) and against
the host twin over image sizes around the kernel's 32 x 8 tiles, every radius and rank, and spikes planted beside the tile seams; the
identities; buffer kinds and refused aliasing; the work buffer regrown; isolation from the other entry points; and the pipeline
render -> ff_gbuffer -> ff_despeckle -> ff_denoise on a real 1-spp frame."""
import ctypes as C

import numpy as np
import pytest

from gpupathtracer_amd import lib, scenes
from gpupathtracer_amd import types as T
import despeckle_ref as R
from despeckle_cases import PLANT_SIZE, RADII, RANKS, SEAMS, SIZES, assert_same, inputs, planted, reference

pytestmark = pytest.mark.gpu

F = np.float32
FLAG = T.DESPECKLE_DEMODULATE_ALBEDO
C2_POSE = dict(yaw=-90.0, pitch=0.0)
BIG = (320, 180)


def check_all_three(tracer, rad, albedo, ids, p):
    got = tracer.despeckle(rad, (albedo, ids), p)
    assert_same(got, reference(rad, albedo, ids, p))
    assert_same(got, lib.despeckle_host(rad, (albedo, ids), p))
    return got


@pytest.mark.parametrize("w,h", SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
def test_reference_and_twin_parity_bit_for_bit(tracer, w, h):
    rad, albedo, ids = inputs(w, h)
    changed = 0
    for r in RADII:
        for rank in RANKS:
            changed += check_all_three(tracer, rad, albedo, ids, lib.despeckle_params(radius=r, rank=rank, min_neighbours=max(rank, 3)))[2]
        check_all_three(tracer, rad, None, ids, lib.despeckle_params(radius=r, rank=1, min_neighbours=1, flags=0, threshold=1.5, floor=0.5))
        check_all_three(tracer, rad, albedo, ids, lib.despeckle_params(radius=r, rank=4, min_neighbours=(2 * r + 1) ** 2 - 1))
    assert changed or w * h <= 64


def test_parity_at_320x180(tracer):
    w, h = BIG
    rad, albedo, ids = inputs(w, h)
    assert len(planted(w, h)) == len(planted(*PLANT_SIZE))
    for r, rank, flags in ((1, 2, FLAG), (2, 1, 0), (3, 4, FLAG)):
        n = check_all_three(tracer, rad, albedo if flags else None, ids, lib.despeckle_params(radius=r, rank=rank, min_neighbours=max(rank, 3), flags=flags))[2]
        assert n > 100


def test_spikes_beside_the_tile_seams(tracer):
    """The noise-free ramp with the planted spikes alone: the pairs of SEAMS see each other only across a seam of the kernel's
    tiles, so with rank 1 a spike survives exactly when the apron delivered its other half."""
    w, h = PLANT_SIZE
    rad, albedo, ids = inputs(w, h, noise=False)
    for r in RADII:
        for rank in RANKS:
            out = check_all_three(tracer, rad, albedo, ids, lib.despeckle_params(radius=r, rank=rank, min_neighbours=max(rank, 3)))[1]
            if rank == 1:
                for (ya, xa), (yb, xb) in SEAMS:
                    apart = max(abs(ya - yb), abs(xa - xb))
                    for y, x in ((ya, xa), (yb, xb)):
                        assert np.array_equal(R.bits(out[y, x]), R.bits(rad[y, x])) == (r >= apart)


def test_identities_on_the_device(tracer):
    w, h = 33, 31
    rad, albedo, ids = inputs(w, h)
    flat = np.empty_like(rad)
    flat[:] = (0.7, -0.0, 3.0)
    for r in RADII:
        for rank in (1, 4):
            p = lib.despeckle_params(radius=r, rank=rank, min_neighbours=rank, threshold=1.0)
            rgb8, out, n = check_all_three(tracer, flat, np.ones_like(albedo), ids, p)
            assert n == 0 and np.array_equal(R.bits(out), R.bits(flat)) and np.array_equal(rgb8, R.to_u8(flat))
    rgb8, out, n = check_all_three(tracer, rad, albedo, ids, lib.despeckle_params(threshold=3.0e38))
    assert n == 0 and np.array_equal(R.bits(out), R.bits(rad)) and np.array_equal(rgb8, R.to_u8(rad))
    for p in (lib.despeckle_params(), lib.despeckle_params(radius=3, rank=4, min_neighbours=6, threshold=1.5, flags=0)):
        base = check_all_three(tracer, rad, albedo, ids, p)
        assert base[2] > 0
        for k in (F(2.0 ** -20), F(2.0 ** 9)):
            scaled = tracer.despeckle(rad * k, (albedo, ids), p)
            assert scaled[2] == base[2] and np.array_equal(R.bits(scaled[1]), R.bits(base[1] * k))
    # non-finite pixels are copied through and are nobody's neighbour
    dirty, bad_albedo = np.array(rad), np.array(albedo)
    dirty[3, 4] = (np.nan, 0.5, 0.25)
    dirty[10, 20] = np.inf
    dirty[20, 5] = (-np.inf, np.nan, 1.0)
    bad_albedo[15, 15] = (0.5, np.nan, 0.5)
    missed = np.array(ids)
    for yx in ((3, 4), (10, 20), (20, 5), (15, 15)):
        missed[yx] = (-1, -1, -1)
    for r in RADII:
        p = lib.despeckle_params(radius=r)
        got = check_all_three(tracer, dirty, bad_albedo, ids, p)
        assert_same(got, tracer.despeckle(dirty, (bad_albedo, missed), p))


def test_buffer_kinds_and_aliasing(tracer):
    import torch
    w, h = 101, 67
    rad, albedo, ids = inputs(w, h)
    p = lib.despeckle_params(radius=2)
    host8, host_out, host_n = check_all_three(tracer, rad, albedo, ids, p)
    assert host_n > 0
    # only the bytes, only the floats, neither (the count still comes)
    got = tracer.despeckle(rad, (albedo, ids), p, want_out=False)
    assert got[1] is None and np.array_equal(got[0], host8) and got[2] == host_n
    got = tracer.despeckle(rad, {"albedo": albedo, "ids": ids}, p, want_rgb8=False)
    assert got[0] is None and np.array_equal(R.bits(got[1]), R.bits(host_out)) and got[2] == host_n
    assert tracer.despeckle(rad, (albedo, ids), p, want_rgb8=False, want_out=False) == (None, None, host_n)
    # device tensors through the same method
    d_rad, d_alb, d_ids = (torch.from_numpy(np.array(a)).cuda() for a in (rad, albedo, ids))
    t8, t_out, t_n = tracer.despeckle(d_rad, (d_alb, d_ids), p)
    assert t8.is_cuda and t_out.is_cuda
    assert_same((t8.cpu().numpy(), t_out.cpu().numpy(), t_n), (host8, host_out, host_n))
    for d, a in ((d_rad, rad), (d_alb, albedo)):
        assert np.array_equal(R.bits(d.cpu().numpy()), R.bits(a))  # (the inputs are left alone)
    assert np.array_equal(d_ids.cpu().numpy(), ids)
    # raw pointers: one output at a time, out_clamped NULL
    d8 = torch.zeros((h, w, 3), dtype=torch.uint8, device="cuda")
    d_out = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    ptrs = (d_rad.data_ptr(), d_alb.data_ptr(), d_ids.data_ptr())
    assert tracer.despeckle_device(w, h, *ptrs, p, d8.data_ptr(), None) == host_n
    assert np.array_equal(d8.cpu().numpy(), host8)
    assert tracer.despeckle_device(w, h, *ptrs, p, None, d_out.data_ptr(), want_count=False) is None
    assert np.array_equal(R.bits(d_out.cpu().numpy()), R.bits(host_out))
    assert tracer.despeckle_device(w, h, *ptrs, p, None, None) == host_n
    # without the flag the albedo may be NULL on the device as well
    q = lib.despeckle_params(radius=2, flags=0)
    d_out.zero_()
    torch.cuda.synchronize()
    n0 = tracer.despeckle_device(w, h, d_rad.data_ptr(), None, d_ids.data_ptr(), q, None, d_out.data_ptr())
    assert_same((None, d_out.cpu().numpy(), n0), reference(rad, None, ids, q))
    # buffers that are only 4-byte aligned
    big = torch.zeros(h * w * 6 + 8, dtype=torch.float32, device="cuda")
    big[1:1 + h * w * 3] = d_rad.reshape(-1)
    big[h * w * 3 + 3:h * w * 6 + 3] = d_alb.reshape(-1)
    b8 = torch.zeros(h * w * 3 + 8, dtype=torch.uint8, device="cuda")
    d_out.zero_()
    torch.cuda.synchronize()
    assert tracer.despeckle_device(w, h, big.data_ptr() + 4, big.data_ptr() + 4 * (h * w * 3 + 3), d_ids.data_ptr(), p, b8.data_ptr() + 1, d_out.data_ptr()) == host_n
    assert np.array_equal(b8.cpu().numpy()[1:1 + h * w * 3].reshape(h, w, 3), host8) and np.array_equal(R.bits(d_out.cpu().numpy()), R.bits(host_out))
    # mixed: device inputs with host outputs, host inputs with device outputs, through the raw entry point
    lib_ = lib.load()
    m8, m_out, m_n = np.zeros((h, w, 3), np.uint8), np.zeros((h, w, 3), np.float32), C.c_uint32(0)
    vp = C.c_void_p
    lib.check(lib_.ff_despeckle(tracer._state, w, h, C.byref(p), vp(ptrs[0]), vp(ptrs[1]), vp(ptrs[2]), 1, m8.ctypes.data, 0, m_out.ctypes.data, 0, C.byref(m_n)))
    assert_same((m8, m_out, m_n.value), (host8, host_out, host_n))
    d8.zero_()
    d_out.zero_()
    torch.cuda.synchronize()
    lib.check(lib_.ff_despeckle(tracer._state, w, h, C.byref(p), rad.ctypes.data, albedo.ctypes.data, ids.ctypes.data, 0, vp(d8.data_ptr()), 1,
                                vp(d_out.data_ptr()), 1, C.byref(m_n)))
    assert_same((d8.cpu().numpy(), d_out.cpu().numpy(), m_n.value), (host8, host_out, host_n))
    # an output on an input or on the other output is refused on the host: nothing is launched, nothing is written
    d_out.fill_(7.0)
    torch.cuda.synchronize()
    for args, words in [((None, ptrs[0]), "radiance_out overlaps radiance_in"), ((None, ptrs[1]), "radiance_out overlaps albedo"),
                        ((None, ptrs[2]), "radiance_out overlaps ids"), ((ptrs[1] + 16, None), "rgb8 overlaps albedo"),
                        ((d_out.data_ptr() + 64, d_out.data_ptr()), "rgb8 overlaps radiance_out")]:
        with pytest.raises(lib.FireflyError) as e:
            tracer.despeckle_device(w, h, *ptrs, p, *args)
        assert e.value.status == T.FF_ERR_INVALID_ARG and words in e.value.message
    assert (d_out.cpu().numpy() == 7.0).all()
    assert np.array_equal(R.bits(d_rad.cpu().numpy()), R.bits(rad)) and np.array_equal(R.bits(d_alb.cpu().numpy()), R.bits(albedo))
    assert np.array_equal(d_ids.cpu().numpy(), ids)


def test_the_work_buffer_regrows(tracer):
    p = lib.despeckle_params(radius=3, rank=2)
    for w, h in (BIG, (33, 9), BIG, (1, 1), PLANT_SIZE):
        rad, albedo, ids = inputs(w, h)
        assert_same(tracer.despeckle(rad, (albedo, ids), p), lib.despeckle_host(rad, (albedo, ids), p))


def test_despeckle_is_not_a_frame(tracer):
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
    assert_same(tracer.despeckle(second[1], gb), reference(second[1], gb["albedo"], gb["ids"], lib.despeckle_params()))
    rad, albedo, ids = inputs(*BIG)            # (a larger image: the work buffer is regrown)
    tracer.despeckle(rad, (albedo, ids), lib.despeckle_params(radius=3))
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
    rad, albedo, ids = inputs(17, 15)
    with lib.Tracer(0) as t:
        p = lib.despeckle_params()
        assert_same(t.despeckle(rad, (albedo, ids), p), lib.despeckle_host(rad, (albedo, ids), p))
        out = np.full(rad.shape, 7.0, np.float32)
        lib_ = lib.load()
        for field, value in [("radius", 4), ("rank", 0), ("min_neighbours", 1), ("threshold", 0.5), ("floor", -1.0), ("flags", 2), ("reserved", 1)]:
            q = lib.despeckle_params(**{field: value})
            assert lib_.ff_despeckle(t._state, 17, 15, C.byref(q), rad.ctypes.data, albedo.ctypes.data, ids.ctypes.data, 0, None, 0, out.ctypes.data, 0,
                                     None) == T.FF_ERR_INVALID_ARG
            assert field in lib_.ff_last_error().decode()
        assert (out == 7.0).all()


def test_pipeline_on_a_real_frame(tracer):
    """A 1-spp frame of the mirror Cornell box with next-event estimation, its G-buffer, the clamp, the denoiser."""
    w, h = 64, 36
    tracer.upload_scene(scenes.cornell_mirror_scene())
    cam = scenes.posed_camera(w, h, position=(0.0, 0.0, 5.0), **C2_POSE)  # (from outside the open front: the light and misses are in view)
    gb = tracer.gbuffer(cam, lib.render_params(w, h))
    rad = tracer.render(cam, lib.render_params(w, h, 8, 1, seed=11, shade_mode=T.SHADE_DIFFUSE_PATH_NEE))[1]
    for p in (lib.despeckle_params(), lib.despeckle_params(radius=2, rank=3, threshold=1.5)):
        rgb8, out, n = check_all_three(tracer, rad, gb["albedo"], gb["ids"], p)
        print(f"radius {p.radius} rank {p.rank}: {n} of {w * h} pixels clamped, mean {out.mean():.5g} of {rad.mean():.5g}")
        l_in, g = R.measure(rad, gb["albedo"], gb["ids"])
        l_out, g_out = R.measure(out, gb["albedo"], gb["ids"])
        assert (g >= 0).sum() > w * h // 2 and np.array_equal(g, g_out)
        assert (l_out[g >= 0] <= l_in[g >= 0]).all()
        miss = gb["ids"][..., 0] < 0
        emitter = ~miss & (gb["ids"][..., 2] == T.BXDF_EMITTER)
        assert miss.any() and emitter.any() and np.array_equal(R.bits(out[miss | emitter]), R.bits(rad[miss | emitter]))
        denoised8, denoised = tracer.denoise(out, gb)
        assert np.isfinite(denoised).all() and denoised8.any()
