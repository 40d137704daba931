"""Start records (csrc/ff_k_shade.h settle_hit<PREPASS>, scatter_start; csrc/ff_kernels.hip trace_bvh_kernel<..., START>; csrc/ff_frame.cpp
render_enqueue): the pre-pass of a frame shades every pixel's stored primary hit once, and on diffuse scenes of up to 32 geometries
every sample of the frame starts from that record inside the shading pass that ended the sample before it.  Nothing a frame
computes may change: every case compares radiance bits, rgb8 bytes and the ray counters of three renderings -
  on:    the default;
  off:   FF_NO_START_RECORDS=1, the kernel that starts every sample from the pixel's raw stored hit;
  brute: FF_TRACE_BRUTE_FORCE, the reference's loop, which traces every segment: its rays_traced must agree, its rays_answered and
         rays_cut_short are zero by construction (tests/test_gpu_properties.py), so those two are compared between on and off.
Scenes the START instantiation does not serve (MIRROR / GLASS surfaces, spheres, interpolated normals, more than 32 geometries, the
job-pool kernel) keep the raw-hit kernel whatever the switch says; they are rendered here all the same, and the kernel's name says
which instantiation ran."""
import numpy as np
import pytest

from gpupathtracer_amd import lib, scenes
from gpupathtracer_amd import types as T
from oracle_lib import oracle_render

pytestmark = pytest.mark.gpu

START_NAME = ", false, 0, false, true>"
W, H = 96, 64
INSIDE = dict(position=(0.0, 0.0, 2.4), yaw=-90.0, pitch=0.0)


def _frame(t, render):
    rgb8, rad = render(t)
    st = t.stats()
    return rgb8.copy(), rad.view(np.uint32).copy(), int(st.rays_traced), int(st.rays_answered), int(st.rays_cut_short), t.kernel_name()


def _on_off(tracer, monkeypatch, render, expect_start=True):
    """render(t) under the default and under FF_NO_START_RECORDS=1: equal in everything but the kernel's name."""
    monkeypatch.delenv("FF_NO_START_RECORDS", raising=False)
    # (every frame on stored hits: whether a one-off 1-spp frame runs a pre-pass depends on the frame before it, which differs
    # between the two renderings here)
    monkeypatch.setenv("FF_REUSE_MIN_SPP", "1")
    tracer.reload_switches()
    on = _frame(tracer, render)
    monkeypatch.setenv("FF_NO_START_RECORDS", "1")
    tracer.reload_switches()
    off = _frame(tracer, render)
    monkeypatch.delenv("FF_NO_START_RECORDS")
    monkeypatch.delenv("FF_REUSE_MIN_SPP")
    tracer.reload_switches()
    assert on[5].endswith(START_NAME) == expect_start, on[5]
    assert not off[5].endswith(START_NAME), off[5]
    assert on[2:5] == off[2:5], (on[2:5], off[2:5])
    assert np.array_equal(on[0], off[0]) and np.array_equal(on[1], off[1])
    return on


def _three(tracer, monkeypatch, cam, params, expect_start=True):
    on = _on_off(tracer, monkeypatch, lambda t: t.render(cam, params), expect_start)
    params.trace_mode = T.TRACE_BRUTE_FORCE
    brute = _frame(tracer, lambda t: t.render(cam, params))
    params.trace_mode = T.TRACE_BVH
    assert brute[2] == on[2] and brute[3] == 0 and brute[4] == 0, (on[2:5], brute[2:5])
    assert np.array_equal(on[0], brute[0]) and np.array_equal(on[1], brute[1])
    return on


@pytest.mark.parametrize("bounces", [1, 2, 8])
def test_sample_and_bounce_counts(tracer, monkeypatch, bounces):
    """C2 from the inside camera: one bounce (every pixel's path ends at its first hit: no item reaches the loop), partial blocks
    (65, 130), one sample, several blocks, blocks of 128 samples (1 100 spp)."""
    tracer.upload_scene(scenes.cornell_wahoo_scene())
    for spp in (1, 2, 64, 65, 130, 1100):
        w, h = (48, 32) if spp == 1100 else (W, H)
        cam = scenes.posed_camera(w, h, **INSIDE)
        on = _three(tracer, monkeypatch, cam, lib.render_params(w, h, bounces, spp, 11))
        assert on[3] > 0  # (primary segments answered from the records)
        assert on[1].any() == (bounces > 1)  # (the emitter is not in view of this camera: a one-bounce frame is black)


def test_emitter_miss_and_culled_pixels(tracer, monkeypatch):
    """A camera that looks at the emitter plane (its pixels end there with the emitter's radiance), one that sees past the open box
    (pixels that hit nothing; the camera is outside the scene's box, so the mask pass culls some of them first), with and without
    the exact cull, at sample counts with and without tail items."""
    tracer.upload_scene(scenes.cornell_wahoo_scene())
    up = scenes.posed_camera(W, H, position=(0.0, 0.0, 1.0), yaw=-90.0, pitch=70.0)
    down = scenes.posed_camera(W, H, position=(0.0, 0.0, 1.0), yaw=-90.0, pitch=-70.0)
    past = scenes.posed_camera(W, H, position=(4.0, 1.0, 7.0), yaw=-118.0, pitch=-8.0)
    far = scenes.posed_camera(W, H, position=(6.0, 2.0, 9.0), yaw=-125.0, pitch=-10.0)
    for cam in (up, down, past, far):
        for bounces, spp in ((5, 3), (4, 70), (3, 200), (2, 1100)):
            _three(tracer, monkeypatch, cam, lib.render_params(W, H, bounces, spp, 3))
    monkeypatch.setenv("FF_NO_PRIMARY_CULL", "1")
    for cam in (up, past):
        _three(tracer, monkeypatch, cam, lib.render_params(W, H, 4, 70, 3))
    monkeypatch.delenv("FF_NO_PRIMARY_CULL")
    # the emitter really is in view of the first camera, and nothing is in view of some pixels of the second
    assert max(tracer.render(c, lib.render_params(W, H, 1, 2, 3))[1].max() for c in (up, down)) > 1.0  # (whichever way pitch counts)
    rgb8, rad = tracer.render(past, lib.render_params(W, H, 4, 8, 3))
    assert (rad.reshape(-1, 3).max(axis=1) == 0).sum() > W * H // 4


@pytest.mark.parametrize("num_parts", [2, 3])
def test_strips_and_parts(tracer, monkeypatch, num_parts):
    """The strips of a multi-part frame hand their last block(s) out as tail items (per-sample storage): those of pixels that end at
    the first hit are answered at the queue, those of the others start every sample from the record.  Each part equals its rows of
    the brute-force frame."""
    tracer.upload_scene(scenes.cornell_wahoo_scene())
    w, h, rows = 96, 72, 8
    for cam in (scenes.posed_camera(w, h, **INSIDE), scenes.posed_camera(w, h, position=(4.0, 1.0, 7.0), yaw=-118.0, pitch=-8.0)):
        for bounces, spp in ((4, 130), (1, 70), (6, 200)):
            p = lib.render_params(w, h, bounces, spp, 8)
            p.trace_mode = T.TRACE_BRUTE_FORCE
            brute = tracer.render(cam, p)[1].view(np.uint32).copy()
            p.trace_mode = T.TRACE_BVH
            for part in range(num_parts):
                on = _on_off(tracer, monkeypatch, lambda t: t.render_strips(cam, p, rows, part, num_parts))
                gy = [(s * num_parts + part) * rows + r for s in range((h + rows - 1) // rows) for r in range(rows)]
                gy = [y for y in gy if y < h]
                assert len(gy) == on[1].shape[0]
                assert np.array_equal(on[1], brute[gy])


def test_scenes_the_start_kernel_does_not_serve(tracer, monkeypatch):
    """MIRROR and GLASS at the first hit, spheres, interpolated normals, more than 32 geometries: the raw-hit kernel, same frames."""
    import sys, os
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import fuzz_parity as fz
    cam = scenes.posed_camera(W, H, **INSIDE)
    for scene in (scenes.cornell_glass_scene(), scenes.cornell_mirror_scene(), scenes.cornell_spheres_scene()):
        tracer.upload_scene(scene)
        _three(tracer, monkeypatch, cam, lib.render_params(W, H, 6, 9, 3), expect_start=False)
    tracer.upload_scene(scenes.cornell_wahoo_scene())
    _three(tracer, monkeypatch, cam, lib.render_params(W, H, 4, 70, 3, T.TRACE_BVH, T.SHADE_DIFFUSE_PATH_SMOOTH), expect_start=False)
    _three(tracer, monkeypatch, cam, lib.render_params(W, H, 1, 1, 0, T.TRACE_BVH, T.SHADE_NORMAL_DEBUG), expect_start=False)
    crowded = fz.rand_scene(np.random.default_rng(3), small=True, crowd=80)
    assert len(crowded) > 32
    tracer.upload_scene(crowded)
    _three(tracer, monkeypatch, scenes.posed_camera(W, H, position=(0.5, 0.2, 4.5), yaw=-95.0, pitch=-4.0), lib.render_params(W, H, 5, 6, 3), expect_start=False)


def test_a_frame_against_the_oracle(tracer, monkeypatch):
    monkeypatch.delenv("FF_NO_START_RECORDS", raising=False)
    tracer.reload_switches()
    scene = scenes.cornell_wahoo_scene()
    cam = scenes.posed_camera(40, 28, **INSIDE)
    p = lib.render_params(40, 28, 8, 4, 17)
    tracer.upload_scene(scene)
    rgb8, rad = tracer.render(cam, p)
    assert tracer.kernel_name().endswith(START_NAME)
    o_rgb8, o_rad = oracle_render(scene, cam, p, threads=16)
    assert np.array_equal(rgb8, o_rgb8) and np.array_equal(rad.view(np.uint32), o_rad.view(np.uint32)) and o_rad.max() > 0


def test_start_records_are_kept_only_for_their_bounce_count_and_shade_mode(monkeypatch):
    """The kept-records rule: the sequence of tests/test_gpu_properties.py test_stored_primary_hits_are_kept_while_camera_and_scene_stay
    (cameras, sizes, sample counts, shade modes, a tile, a transform update, a fresh upload), with frames of one camera that differ
    only in `bounces` added - one bounce, then eight, then one: the class of a pixel depends on it, a stale class would show as wrong
    bits - and a pixel jitter.  Start records on, off, and nothing kept (FF_NO_PRIMARY_CACHE=1) give the same frames and counts."""
    scene = scenes.cornell_wahoo_scene()
    inside = scenes.posed_camera(160, 96, **INSIDE)
    outside = scenes.posed_camera(160, 96, position=(6.0, 2.0, 9.0), yaw=-125.0, pitch=-10.0)
    steps = [("a", inside, lib.render_params(160, 96, 8, 1, 5)), ("a again", inside, lib.render_params(160, 96, 8, 1, 6)),
             ("a third", inside, lib.render_params(160, 96, 8, 1, 8)), ("a 70 spp", inside, lib.render_params(160, 96, 4, 70, 7)),
             ("a one bounce", inside, lib.render_params(160, 96, 1, 70, 7)), ("a eight bounces", inside, lib.render_params(160, 96, 8, 6, 7)),
             ("a one bounce again", inside, lib.render_params(160, 96, 1, 3, 7)), ("a two bounces", inside, lib.render_params(160, 96, 2, 3, 7)),
             ("a smooth", inside, lib.render_params(160, 96, 4, 3, 7, T.TRACE_BVH, T.SHADE_DIFFUSE_PATH_SMOOTH)),
             ("a flat again", inside, lib.render_params(160, 96, 4, 3, 7)), ("b", outside, lib.render_params(160, 96, 8, 1, 5)),
             ("b 130 spp", outside, lib.render_params(160, 96, 5, 130, 2)), ("b one bounce", outside, lib.render_params(160, 96, 1, 130, 2)),
             ("b again", outside, lib.render_params(160, 96, 8, 3, 9)), ("b 200 spp", outside, lib.render_params(160, 96, 3, 200, 4)),
             ("a small", scenes.posed_camera(96, 64, **INSIDE), lib.render_params(96, 64, 6, 2, 1)),
             ("a back", inside, lib.render_params(160, 96, 8, 1, 5))]

    def run(env):
        for k in ("FF_NO_PRIMARY_CACHE", "FF_NO_START_RECORDS"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        out = []
        with lib.Tracer(0) as t:
            t.upload_scene(scene)
            for name, cam, p in steps:
                rgb8, rad = t.render(cam, p)
                st = t.stats()
                out.append((name, rad.view(np.uint32).copy(), st.rays_traced, st.rays_answered, st.rays_cut_short, rgb8.copy()))
            t.set_pixel_jitter(0.25, 0.625)
            for bounces in (4, 1, 4):
                rgb8, rad = t.render(inside, lib.render_params(160, 96, bounces, 5, 3))
                st = t.stats()
                out.append((f"jittered {bounces}", rad.view(np.uint32).copy(), st.rays_traced, st.rays_answered, st.rays_cut_short, rgb8.copy()))
            t.set_pixel_jitter(0.0, 0.0)
            tile = t.render_tile(inside, lib.render_params(160, 96, 4, 2, 3), 40, 24, 80, 48)
            out.append(("tile", tile[1].view(np.uint32).copy(), 0, 0, 0, tile[0].copy()))
            full = t.render(inside, lib.render_params(160, 96, 4, 2, 3))
            st = t.stats()
            out.append(("full after tile", full[1].view(np.uint32).copy(), st.rays_traced, st.rays_answered, st.rays_cut_short, full[0].copy()))
            assert np.array_equal(out[-2][1], out[-1][1][24:72, 40:120])
            shifted = scenes.Scene()
            shifted.add_mesh(scenes.load_mesh("wahoo"), (0.4, -2.4, 0.3), (0, 25, 0), (0.28, 0.28, 0.28), scenes.make_bxdf(T.BXDF_DIFFUSE, albedo=(1, 0, 0)))
            shifted.add_mesh(scenes.load_mesh("cube"), (1.2, -2.0, 0.6), (0, 10, 0), (1, 1, 1), scenes.make_bxdf(T.BXDF_DIFFUSE, albedo=(0.75, 0.75, 0.75)))
            scenes._box(shifted).finalize()
            t.update_transforms(shifted)
            upd = t.render(inside, lib.render_params(160, 96, 4, 2, 3))
            st = t.stats()
            out.append(("after transform update", upd[1].view(np.uint32).copy(), st.rays_traced, st.rays_answered, st.rays_cut_short, upd[0].copy()))
            t.upload_scene(scene)
            back = t.render(inside, lib.render_params(160, 96, 4, 2, 3))
            st = t.stats()
            out.append(("after re-upload", back[1].view(np.uint32).copy(), st.rays_traced, st.rays_answered, st.rays_cut_short, back[0].copy()))
        with lib.Tracer(0) as t2:
            t2.upload_scene(shifted)
            fresh = t2.render(inside, lib.render_params(160, 96, 4, 2, 3))
            assert np.array_equal(out[-2][1], fresh[1].view(np.uint32)) and out[-2][2] == t2.stats().rays_traced
        return out

    on = run({})
    off = run({"FF_NO_START_RECORDS": "1"})
    none = run({"FF_NO_PRIMARY_CACHE": "1"})
    for a, b, c in zip(on, off, none):
        assert np.array_equal(a[1], b[1]) and np.array_equal(a[5], b[5]) and a[2:5] == b[2:5], (a[0], a[2:5], b[2:5])
        assert np.array_equal(a[1], c[1]) and a[2] == c[2] and a[4] == c[4], a[0]
    assert on[-3][0] == "full after tile" and np.array_equal(on[-1][1], on[-3][1])  # (the re-uploaded scene is the first one)
    with lib.Tracer(0) as t:
        t.upload_scene(scene)
        for (name, cam, p), ref in zip(steps, on):
            p.trace_mode = T.TRACE_BRUTE_FORCE
            brute = t.render(cam, p)
            assert np.array_equal(brute[1].view(np.uint32), ref[1]) and t.stats().rays_traced == ref[2], name
            p.trace_mode = T.TRACE_BVH


def test_job_pool_kernel_against_the_default(monkeypatch):
    """FF_POOL=1 stays on the raw hits (its pre-pass writes no start records); the default runs on the records: same frames."""
    cam = scenes.posed_camera(112, 72, **INSIDE)
    p = lib.render_params(112, 72, 8, 70, 5)

    def frame(env):
        monkeypatch.delenv("FF_POOL", raising=False)
        monkeypatch.delenv("FF_NO_START_RECORDS", raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        with lib.Tracer(0) as t:
            t.upload_scene(scenes.cornell_wahoo_scene())
            return _frame(t, lambda tt: tt.render(cam, p))

    ref = frame({"FF_POOL": "0"})
    pool = frame({"FF_POOL": "1"})
    monkeypatch.delenv("FF_POOL")
    assert ref[5].endswith(START_NAME) and "trace_pool_kernel" in pool[5]
    assert ref[2:5] == pool[2:5]
    assert np.array_equal(ref[0], pool[0]) and np.array_equal(ref[1], pool[1])
