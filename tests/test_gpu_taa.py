"""ff_taa on the GPU: agreement with the float64 numpy reference (tests/taa_ref.py) at rest, under camera motion and under rigid
object motion in both sample modes with the clamp on and off, motion vectors, resets, scaling, isolation from the other entry
points, repeatability and buffer kinds, and the anti-aliasing it buys on the C2 scene at rest."""
import functools

import numpy as np
import pytest

from gpupathtracer_amd import lib, scenes
from gpupathtracer_amd import types as T
from taa_ref import TaaRef
from temporal_ref import ray_matrix, scene_models

pytestmark = pytest.mark.gpu

W, H = 160, 90
# three poses a few pixels apart (the back wall moves ~2-3 px between them)
POSES = [((0.0, 0.0, 2.4), -90.0), ((0.06, -0.04, 2.4), -89.3), ((0.1, -0.02, 2.37), -88.8)]
CUBE = 1


def cam(pose, w=W, h=H):
    (x, y, z), yaw = pose
    return scenes.posed_camera(w, h, position=(x, y, z), yaw=yaw, pitch=0.0)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def synthetic_radiance(seed, w=W, h=H):
    """test_gpu_temporal's seeded radiance: a smooth image times noise, a few pixels far brighter than their neighbours."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    smooth = np.stack([0.4 + 0.3 * np.sin(xx / 17.0), 0.3 + 0.2 * np.cos(yy / 11.0), 0.2 + 0.001 * xx], -1)
    rad = smooth * rng.uniform(0.3, 1.7, size=(h, w, 3)) * np.where(rng.random((h, w, 1)) < 0.02, 8.0, 1.0)
    return rad.astype(np.float32)


def wahoo_with_cube_at(cube_position):
    s = scenes.Scene()
    s.add_mesh(scenes.load_mesh("wahoo"), (0, -2.4, 0), (0, 0, 0), (0.28, 0.28, 0.28), scenes.make_bxdf(T.BXDF_DIFFUSE, albedo=(1, 0, 0)))
    s.add_mesh(scenes.load_mesh("cube"), cube_position, (0, 0, 0), (1, 1, 1), scenes.make_bxdf(T.BXDF_DIFFUSE, albedo=(0.75, 0.75, 0.75)))
    return scenes._box(s).finalize()


CUBE_POSITIONS = [(0.6, -0.6, -0.5), (0.52, -0.6, -0.5), (0.47, -0.57, -0.5)]


@functools.lru_cache(maxsize=None)
def scene_of(name):
    if name.startswith("cube"):
        return wahoo_with_cube_at(CUBE_POSITIONS[int(name[4:])])
    return getattr(scenes, name)()


@functools.lru_cache(maxsize=None)
def guides(scene_name, pose_index, jitter, w=W, h=H):
    with lib.Tracer(0) as t:
        t.upload_scene(scene_of(scene_name))
        t.set_pixel_jitter(*jitter)
        return t.gbuffer(cam(POSES[pose_index], w, h), lib.render_params(w, h))


# name -> the (scene, pose) of each call; the scenes of one sequence share their geometries (update_transforms between calls)
SEQUENCES = {
    "at_rest": [("cornell_wahoo_scene", 0)] * 3,
    "sliding": [("cornell_wahoo_scene", 0), ("cornell_wahoo_scene", 1), ("cornell_wahoo_scene", 2)],
    "cube_moved": [("cube0", 0), ("cube1", 0), ("cube2", 1)],
}


def jitter_of(i):
    return lib.jitter_sequence(i, 16)


def run_sequence(tracer, seq, p, scale=1.0, between=None, upload=True):
    """taa_reset, then one call per (scene, pose) of the sequence (call i on synthetic_radiance(100 + i), jitter_of(i))
    -> list of (rgb8, radiance, motion, length)."""
    calls = SEQUENCES[seq]
    if upload:
        tracer.upload_scene(scene_of(calls[0][0]))
    tracer.taa_reset()
    outs = []
    for i, (scene_name, k) in enumerate(calls):
        if i > 0 and scene_name != calls[i - 1][0]:
            tracer.update_transforms(scene_of(scene_name))
        gb = guides(scene_name, k, jitter_of(i))
        rgb8, out = tracer.taa(synthetic_radiance(100 + i) * np.float32(scale), gb, cam(POSES[k]), p)
        motion, length = tracer.taa_history()
        outs.append((rgb8, out, motion, length))
        if between is not None:
            between(i)
    return outs


FLAGS = [0, T.TAA_BILINEAR, T.TAA_NO_CLAMP, T.TAA_BILINEAR | T.TAA_NO_CLAMP]


@pytest.mark.parametrize("seq", sorted(SEQUENCES))
@pytest.mark.parametrize("flags", FLAGS)
def test_matches_the_numpy_reference(tracer, seq, flags):
    p = lib.taa_params(flags=flags, alpha_min=0.2, gamma=1.25)
    ref = TaaRef()
    outs = run_sequence(tracer, seq, p)
    for i, ((scene_name, k), (rgb8, out, motion, length)) in enumerate(zip(SEQUENCES[seq], outs)):
        gb = guides(scene_name, k, jitter_of(i))
        r = ref.step(synthetic_radiance(100 + i), gb, cam(POSES[k]), scene_models(scene_of(scene_name)), p)
        excused = r["tainted"]
        err = (np.abs(out.astype(np.float64) - r["out"]) / np.maximum(np.abs(r["out"]), 0.1)).max(-1)
        merr = np.abs(motion - r["motion"]).max(-1)
        print(f"{seq} flags {flags} call {i}: max rel err {err[~excused].max():.3g}, motion err {merr[~excused].max():.3g}, "
              f"near {r['near'].sum()}, excused {excused.sum()}, valid {r['valid'].mean():.3f}")
        assert excused.mean() <= (0.0 if seq == "at_rest" else 0.1), excused.mean()  # (measured: at most 5.6 %, Catmull-Rom's 16 taps)
        assert err[~excused].max() <= 1e-3, (i, err[~excused].max(), np.argwhere((err > 1e-3) & ~excused)[:5])
        assert merr[~excused].max() <= 2e-3, (i, merr[~excused].max())
        assert np.array_equal(length[~excused], r["length"][~excused].astype(np.float32))
        if seq == "at_rest":
            assert not motion.any()
    assert r["length"].max() == 3 and r["valid"].mean() > 0.5


def test_motion_follows_the_projection_and_cancels_the_jitter(tracer):
    outs = run_sequence(tracer, "sliding", lib.taa_params())
    assert not outs[0][2].any()  # the first call after a reset has no motion
    motion = outs[1][2]
    gb = guides("cornell_wahoo_scene", 1, jitter_of(1))
    prev, now = cam(POSES[0]), cam(POSES[1])
    x = np.concatenate([gb["position"].astype(np.float64), np.ones((H, W, 1))], -1)

    def P(c):
        q = x @ np.linalg.inv(ray_matrix(c)).T
        return np.stack([(q[..., 0] / q[..., 3] + 1) / 2 * c.m_screenWidth, (1 - q[..., 1] / q[..., 3]) / 2 * c.m_screenHeight], -1)

    hit = gb["ids"][..., 0] >= 0
    expect = P(prev) - P(now)
    assert hit.mean() > 0.9 and np.abs(motion[hit] - expect[hit]).max() <= 1e-3
    assert np.abs(motion[hit]).max() > 1.0  # (the camera did move)
    # P(now) is the jittered pixel: the motion is the surface's, not the jitter's
    ys, xs = np.mgrid[0:H, 0:W]
    jx, jy = jitter_of(1)
    assert np.abs(P(now)[hit] - np.stack([xs + jx, ys + jy], -1)[hit]).max() <= 1e-3


def test_resets_and_mesh_updates_match_a_fresh_state(tracer):
    p = lib.taa_params()
    scene_name = "cornell_spheres_scene"
    gb = guides(scene_name, 2, jitter_of(5))
    rad = synthetic_radiance(7)
    c = cam(POSES[2])
    with lib.Tracer(0) as fresh:
        fresh.upload_scene(scene_of(scene_name))
        f8, f = fresh.taa(rad, gb, c, p)
        fm, fl = fresh.taa_history()
        small_gb = fresh.gbuffer(cam(POSES[2], 96, 54), lib.render_params(96, 54))
        s8, s = fresh.taa(synthetic_radiance(7, 96, 54), small_gb, cam(POSES[2], 96, 54), p)  # (a change of size starts afresh)
    with lib.Tracer(0) as fresh_small:
        fresh_small.upload_scene(scene_of(scene_name))
        s8b, sb = fresh_small.taa(synthetic_radiance(7, 96, 54), small_gb, cam(POSES[2], 96, 54), p)
    assert np.array_equal(s8, s8b) and np.array_equal(bits(s), bits(sb))

    def history(scene_calls=2):
        tracer.upload_scene(scene_of(scene_name))
        tracer.taa_reset()
        for i in range(scene_calls):
            tracer.taa(synthetic_radiance(60 + i), guides(scene_name, i, jitter_of(i)), cam(POSES[i]), p)

    def same_as_fresh(o8, o):
        assert np.array_equal(o8, f8) and np.array_equal(bits(o), bits(f))
        m, ln = tracer.taa_history()
        assert np.array_equal(bits(m), bits(fm)) and np.array_equal(bits(ln), bits(fl))

    history()
    tracer.taa_reset()
    same_as_fresh(*tracer.taa(rad, gb, c, p))
    history()
    o8, o = tracer.taa(synthetic_radiance(7, 96, 54), small_gb, cam(POSES[2], 96, 54), p)
    assert np.array_equal(o8, s8b) and np.array_equal(bits(o), bits(sb))
    history()
    tracer.upload_scene(scene_of(scene_name))
    same_as_fresh(*tracer.taa(rad, gb, c, p))
    # ff_update_mesh(g) restarts geometry g alone (the cube, geometry 0 of this scene); the rest continues at rest
    tracer.taa(rad, gb, c, p)
    tracer.update_mesh(0, scenes.load_mesh("cube"))
    tracer.taa(rad, gb, c, p)
    _, length = tracer.taa_history()
    cube = gb["ids"][..., 0] == 0
    assert cube.sum() > 100
    assert (length[cube] == 1).all() and (length[~cube] == 3).all()
    tracer.upload_scene(scene_of(scene_name))  # (the original mesh back for later tests)


def test_scaling_the_input_scales_the_output_without_clamp(tracer):
    for flags in (T.TAA_NO_CLAMP, T.TAA_NO_CLAMP | T.TAA_BILINEAR):
        p = lib.taa_params(flags=flags)
        a = run_sequence(tracer, "sliding", p)
        b = run_sequence(tracer, "sliding", p, scale=4.0)
        for (_, o1, m1, l1), (_, o4, m4, l4) in zip(a, b):
            assert np.allclose(o4, 4.0 * o1.astype(np.float64), rtol=1e-6, atol=0)
            assert np.array_equal(bits(m1), bits(m4)) and np.array_equal(l1, l4)


def _viewer_frames(interleave):
    """render (1 spp twice at rest, 64 spp, a jittered frame), gbuffer, denoise, denoise_temporal, progressive frames; with
    `interleave`, an ff_taa call before and after each step."""
    scene_name = "cornell_wahoo_scene"
    c = cam(POSES[1])
    out = []
    with lib.Tracer(0) as t:
        t.upload_scene(scene_of(scene_name))
        t.set_collect_stats(True)
        k = [0]

        def taa():
            if interleave:
                k[0] += 1
                t.taa(synthetic_radiance(300 + k[0]), guides(scene_name, k[0] % 3, jitter_of(k[0])), cam(POSES[k[0] % 3]))

        def record(name, *arrays):
            st = t.stats()
            out.append((name, [bits(a).copy() if a.dtype != np.uint8 else a.copy() for a in arrays],
                        (st.rays_traced, st.rays_answered, st.rays_cut_short, st.kernel_launches)))

        for name, spp in (("1 spp", 1), ("1 spp at rest", 1), ("64 spp", 64)):
            taa()
            record(name, *t.render(c, lib.render_params(W, H, 8, spp, 5)))
            taa()
        t.set_pixel_jitter(*jitter_of(3))
        taa()
        record("jittered", *t.render(c, lib.render_params(W, H, 8, 1, 6)))
        gb = t.gbuffer(c, lib.render_params(W, H))
        t.set_pixel_jitter(0.0, 0.0)
        taa()
        record("gbuffer", *(gb[n] for n in sorted(gb)))
        _, rad = t.render(c, lib.render_params(W, H, 8, 1, 7))
        taa()
        record("denoise", *t.denoise(rad, gb))
        for i in range(3):
            taa()
            record(f"temporal {i}", *t.denoise_temporal(synthetic_radiance(400 + i), guides(scene_name, i, (0.0, 0.0)), cam(POSES[i])))
            record(f"temporal history {i}", *t.temporal_history())
        for f in range(3):
            taa()
            record(f"progressive {f}", *t.render_progressive(c, lib.render_params(W, H, 8, 1, 11), f))
    return out


def test_isolation_from_the_other_entry_points(tracer):
    plain, mixed = _viewer_frames(False), _viewer_frames(True)
    for (name, a, sa), (_, b, sb) in zip(plain, mixed):
        assert all(np.array_equal(x, y) for x, y in zip(a, b)), name
        assert sa == sb, (name, sa, sb)
    # and the other entry points between ff_taa calls change no bit of them
    p = lib.taa_params()
    alone = run_sequence(tracer, "sliding", p)

    def others(i):
        c = cam(POSES[i])
        tracer.render(c, lib.render_params(W, H, 4, 1, 9))
        gb = tracer.gbuffer(c, lib.render_params(W, H))
        tracer.denoise(synthetic_radiance(50 + i), gb)
        tracer.denoise_temporal(synthetic_radiance(60 + i), gb, c)
        tracer.render_progressive(c, lib.render_params(W, H, 4, 1, 9), i)

    mixed = run_sequence(tracer, "sliding", p, between=others)
    for x, y in zip(alone, mixed):
        assert np.array_equal(x[0], y[0]) and all(np.array_equal(bits(u), bits(v)) for u, v in zip(x[1:], y[1:]))


def test_repeatable_host_equals_device_and_in_place(tracer):
    import torch
    p = lib.taa_params()
    with lib.Tracer(0) as other:
        a = run_sequence(other, "sliding", p)
    b = run_sequence(tracer, "sliding", p)
    for x, y in zip(a, b):
        assert np.array_equal(x[0], y[0]) and all(np.array_equal(bits(u), bits(v)) for u, v in zip(x[1:], y[1:]))
    tracer.taa_reset()
    d8 = torch.zeros((H, W, 3), dtype=torch.uint8, device="cuda")
    d_out = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")
    for i, (scene_name, k) in enumerate(SEQUENCES["sliding"]):
        gb = guides(scene_name, k, jitter_of(i))
        d_pos = torch.from_numpy(np.ascontiguousarray(gb["position"])).cuda()
        d_ids = torch.from_numpy(np.ascontiguousarray(gb["ids"])).cuda()
        d_rad = torch.from_numpy(synthetic_radiance(100 + i)).cuda()
        torch.cuda.synchronize()
        in_place = i >= 1
        tracer.taa_device(cam(POSES[k]), W, H, d_rad.data_ptr(), d_pos.data_ptr(), d_ids.data_ptr(), p, rgb8_ptr=d8.data_ptr(),
                          radiance_out_ptr=d_rad.data_ptr() if in_place else d_out.data_ptr())
        got = (d_rad if in_place else d_out).cpu().numpy()
        assert np.array_equal(d8.cpu().numpy(), b[i][0]) and np.array_equal(bits(got), bits(b[i][1])), i
    motion, length = tracer.taa_history()
    assert np.array_equal(bits(motion), bits(b[2][2])) and np.array_equal(bits(length), bits(b[2][3]))


def test_quality_at_rest_on_c2(tracer):
    """C2 at 160x90, NORMAL_DEBUG frames (|normal| per channel, exact per ray): against S, the mean of ff_gbuffer-derived images over a
    16x16 grid of jitters (the pixel's box-filtered image), 32 frames of ff_jitter_sequence(f, 16) through ff_taa must reach 0.35 of
    the unjittered frame's MSE and the progressive mean of 16 jittered frames 0.15 of it (DESIGN.md section 8 row 7 reports the
    measured factors)."""
    tracer.upload_scene(scenes.cornell_wahoo_scene())
    c = cam(POSES[0])
    dbg = lib.render_params(W, H, 1, 1, 1, shade_mode=T.SHADE_NORMAL_DEBUG)

    def image_of(gb):
        return np.where((gb["ids"][..., 0] >= 0)[..., None], np.abs(gb["normal"].astype(np.float64)), 0.0)

    try:
        S = np.zeros((H, W, 3))
        for i in range(16):
            for j in range(16):
                tracer.set_pixel_jitter((i + 0.5) / 16, (j + 0.5) / 16)
                S += image_of(tracer.gbuffer(c, lib.render_params(W, H)))
        S /= 256
        tracer.set_pixel_jitter(0.0, 0.0)
        _, plain = tracer.render(c, dbg)
        tracer.taa_reset()
        acc = np.zeros((H, W, 3))
        for f in range(32):
            tracer.set_pixel_jitter(*lib.jitter_sequence(f, 16))
            _, frame = tracer.render(c, dbg)
            gb = tracer.gbuffer(c, lib.render_params(W, H))
            assert np.array_equal(bits(frame), bits(image_of(gb).astype(np.float32)))
            if f < 16:
                acc += frame
            _, taa = tracer.taa(frame, gb, c)
    finally:
        tracer.set_pixel_jitter(0.0, 0.0)
    mse = lambda a: float(np.mean((a.astype(np.float64) - S) ** 2))  # noqa: E731
    f_taa, f_mean = mse(taa) / mse(plain), mse(acc / 16) / mse(plain)
    print(f"C2 160x90 at rest: MSE against the 16x16-jitter mean: unjittered {mse(plain):.4g}, TAA 32 frames {mse(taa):.4g} "
          f"(factor {f_taa:.3f}), progressive mean of 16 jittered frames {mse(acc / 16):.4g} (factor {f_mean:.3f})")
    assert f_taa <= 0.35, f_taa
    assert f_mean <= 0.15, f_mean
