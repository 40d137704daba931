"""ff_taa_upscale on the GPU: the exact reconstruction of a full-resolution image from a cycle of jittered half-resolution frames,
bit equality with ff_taa at equal sizes, agreement with the numpy reference (tests/taa_upscale_ref.py) at rest, under camera motion
and under rigid object motion at three size ratios, the history's lifetime and its isolation from the other histories, the
same-geometry rule, non-finite input, repeatability and buffer kinds, every refused call, and the detail it recovers on a texture
no single low frame carries."""
import ctypes as C
import functools

import numpy as np
import pytest

from gpupathtracer_amd import lib, scenes
from gpupathtracer_amd import types as T
from taa_upscale_ref import SPATIAL, TaaUpscaleRef
from temporal_ref import scene_models
from upscale_ref import bilinear_ref

pytestmark = pytest.mark.gpu

W, H = 160, 90
LO = (80, 45)
# test_gpu_taa.py's poses, scenes and sequences (copied, not imported)
POSES = [((0.0, 0.0, 2.4), -90.0), ((0.06, -0.04, 2.4), -89.3), ((0.1, -0.02, 2.37), -88.8)]
BACK_WALL = 1  # geometry index in scenes.cornell_spheres_scene
HALVES = [(0.0, 0.0), (0.5, 0.0), (0.0, 0.5), (0.5, 0.5)]


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


SEQUENCES = {
    "at_rest": [("cornell_wahoo_scene", 0)] * 3,
    "sliding": [("cornell_wahoo_scene", 0), ("cornell_wahoo_scene", 1), ("cornell_wahoo_scene", 2)],
    "cube_moved": [("cube0", 0), ("cube1", 0), ("cube2", 1)],
}
FLAGS = [0, T.TAA_BILINEAR, T.TAA_NO_CLAMP, T.TAA_BILINEAR | T.TAA_NO_CLAMP]


def jitter_of(i):
    return lib.jitter_sequence(i, 16)


def params_of(flags, jitter):
    return lib.taa_upscale_params(flags=flags, alpha_min=0.2, gamma=1.25, lo_jitter=jitter)


def run_sequence(tracer, seq, flags, lo=LO, hi=(W, H), between=None, upload=True, seed=100):
    """taa_upscale_reset, then one call per (scene, pose) of the sequence: call i on synthetic_radiance(seed + i) at the low size with
    the low G-buffer under jitter_of(i) -> list of (rgb8, radiance, motion, length)."""
    calls = SEQUENCES[seq]
    if upload:
        tracer.upload_scene(scene_of(calls[0][0]))
    tracer.taa_upscale_reset()
    outs = []
    for i, (scene_name, k) in enumerate(calls):
        if i > 0 and scene_name != calls[i - 1][0]:
            tracer.update_transforms(scene_of(scene_name))
        j = jitter_of(i)
        rgb8, out = tracer.taa_upscale(synthetic_radiance(seed + i, *lo), guides(scene_name, k, j, *lo), guides(scene_name, k, (0.0, 0.0), *hi),
                                       cam(POSES[k], *hi), params_of(flags, j))
        motion, length = tracer.taa_upscale_history()
        outs.append((rgb8, out, motion, length))
        if between is not None:
            between(i)
    return outs


def same_bits(x, y):
    return np.array_equal(x[0], y[0]) and all(np.array_equal(bits(u), bits(v)) for u, v in zip(x[1:], y[1:]))


@functools.lru_cache(maxsize=None)
def target_image():
    """A seeded float32 image in [0.5, 1).  (From the second call on, a pixel's first sample c meets the spatial estimate h the call
    before stored with length 0, at alpha = 1: o = h + (c - h), which is c when c - h is exact, as it is for h / 2 <= c <= 2 h.)"""
    return np.random.default_rng(5).uniform(0.5, 1.0, size=(H, W, 3)).astype(np.float32)


@pytest.mark.parametrize("flags", [T.TAA_NO_CLAMP, T.TAA_NO_CLAMP | T.TAA_BILINEAR])
def test_a_cycle_of_half_resolution_frames_rebuilds_the_image_exactly(tracer, flags):
    tracer.upload_scene(scene_of("cornell_wahoo_scene"))
    tracer.taa_upscale_reset()
    gb = guides("cornell_wahoo_scene", 0, (0.0, 0.0))
    target = target_image()
    c = cam(POSES[0])
    done = np.zeros((H, W), bool)
    for call in range(8):
        jx, jy = HALVES[call % 4]
        a, b = int(2 * jx), int(2 * jy)
        _, out = tracer.taa_upscale(target[b::2, a::2], {"ids": gb["ids"][b::2, a::2]}, gb, c, lib.taa_upscale_params(flags=flags, lo_jitter=(jx, jy)))
        motion, length = tracer.taa_upscale_history()
        done[b::2, a::2] = True
        assert np.array_equal(bits(out[done]), bits(target[done])), call
        assert not motion.any()
        if call == 3:
            assert done.all() and (length == 1).all()
    assert np.array_equal(bits(out), bits(target)) and (length == 2).all()


@pytest.mark.parametrize("seq", sorted(SEQUENCES))
@pytest.mark.parametrize("flags", FLAGS)
def test_equal_sizes_without_jitter_are_ff_taa_bit_for_bit(tracer, seq, flags):
    calls = SEQUENCES[seq]
    tracer.upload_scene(scene_of(calls[0][0]))
    tracer.taa_reset()
    tracer.taa_upscale_reset()
    for i, (scene_name, k) in enumerate(calls):
        if i > 0 and scene_name != calls[i - 1][0]:
            tracer.update_transforms(scene_of(scene_name))
        gb = guides(scene_name, k, jitter_of(i))
        rad = synthetic_radiance(100 + i)
        a = tracer.taa(rad, gb, cam(POSES[k]), lib.taa_params(flags=flags, alpha_min=0.2, gamma=1.25)) + tracer.taa_history()
        b = tracer.taa_upscale(rad, gb, gb, cam(POSES[k]), params_of(flags, (0.0, 0.0))) + tracer.taa_upscale_history()
        assert same_bits(a, b), i
    assert a[3].max() == 3


@pytest.mark.parametrize("seq", sorted(SEQUENCES))
@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("sizes", [((80, 45), (160, 90)), ((54, 30), (162, 90)), ((107, 61), (160, 90))])
def test_matches_the_numpy_reference(tracer, seq, flags, sizes):
    lo, hi = sizes
    ref = TaaUpscaleRef()
    outs = run_sequence(tracer, seq, flags, lo, hi)
    for i, ((scene_name, k), (rgb8, out, motion, length)) in enumerate(zip(SEQUENCES[seq], outs)):
        j = jitter_of(i)
        r = ref.step(synthetic_radiance(100 + i, *lo), guides(scene_name, k, j, *lo)["ids"], guides(scene_name, k, (0.0, 0.0), *hi), cam(POSES[k], *hi),
                     scene_models(scene_of(scene_name)), params_of(flags, j))
        excused = r["tainted"]
        err = (np.abs(out.astype(np.float64) - r["out"]) / np.maximum(np.abs(r["out"]), 0.1)).max(-1)
        merr = np.abs(motion - r["motion"]).max(-1)
        lerr = np.abs(length - r["length"]) / np.maximum(r["length"], 1e-30)
        print(f"{seq} flags {flags} {lo}->{hi} call {i}: max rel err {err[~excused].max():.3g}, motion err {merr[~excused].max():.3g}, length err "
              f"{lerr[~excused].max():.3g}, excused share {excused.mean():.4f}, valid {r['valid'].mean():.3f}, cases {np.bincount(r['case'].ravel(), minlength=4)}")
        assert excused.mean() <= (0.0 if seq == "at_rest" else 0.1), excused.mean()  # (ff_taa's cap: same poses, G-buffers and taps)
        assert err[~excused].max() <= 1e-3, (i, err[~excused].max(), np.argwhere((err > 1e-3) & ~excused)[:5])
        assert merr[~excused].max() <= 2e-3, (i, merr[~excused].max())
        assert lerr[~excused].max() <= 1e-6, (i, lerr[~excused].max())
        if seq == "at_rest":
            assert not motion.any()
    assert r["valid"].mean() > 0.5


def test_first_calls_start_afresh(tracer):
    """After a reset, a change of either size and upload_scene: length <= k everywhere (no history was read) and no motion."""
    scene_name = "cornell_wahoo_scene"

    def fresh(lo, hi, i):
        j = jitter_of(i)
        p = params_of(0, j)
        g_lo, g_hi = guides(scene_name, 1, j, *lo), guides(scene_name, 1, (0.0, 0.0), *hi)
        tracer.taa_upscale(synthetic_radiance(7, *lo), g_lo, g_hi, cam(POSES[1], *hi), p)
        motion, length = tracer.taa_upscale_history()
        k = TaaUpscaleRef().step(synthetic_radiance(7, *lo), g_lo["ids"], g_hi, cam(POSES[1], *hi), scene_models(scene_of(scene_name)), p)["k"]
        assert (length <= k).all() and length.max() > 0 and not motion.any()

    def history():
        run_sequence(tracer, "sliding", 0)
        assert tracer.taa_upscale_history()[1].max() > 1 and tracer.taa_upscale_history()[0].any()

    history()
    tracer.taa_upscale_reset()
    fresh(LO, (W, H), 3)
    history()
    fresh((54, 30), (W, H), 3)  # (the low size alone changed)
    fresh((54, 30), (162, 90), 4)  # (the high size alone changed)
    history()
    tracer.upload_scene(scene_of(scene_name))
    fresh(LO, (W, H), 5)


def test_isolation_from_the_other_histories():
    scene_name = "cornell_wahoo_scene"
    with lib.Tracer(0) as t:
        t.upload_scene(scene_of(scene_name))
        t.set_collect_stats(True)

        def others_sequence(interleave):
            t.taa_reset()
            t.temporal_reset()
            t.taa_upscale_reset()
            out = []
            for i in range(3):
                c = cam(POSES[i])
                if interleave:
                    j, k = jitter_of(i + 1), (i + 1) % 3
                    t.taa_upscale(synthetic_radiance(300 + i, *LO), guides(scene_name, k, j, *LO), guides(scene_name, k, (0.0, 0.0)), cam(POSES[k]),
                                  params_of(0, j))
                out.append(t.taa(synthetic_radiance(100 + i), guides(scene_name, i, jitter_of(i)), c) + t.taa_history())
                out.append(t.denoise_temporal(synthetic_radiance(400 + i), guides(scene_name, i, (0.0, 0.0)), c) + t.temporal_history())
            return out

        for x, y in zip(others_sequence(False), others_sequence(True)):
            assert same_bits(x, y)
        # the reverse: ff_taa and ff_denoise_temporal between ff_taa_upscale calls change no bit of them, and FfStats stays
        alone = run_sequence(t, "sliding", 0, upload=False)
        t.render(cam(POSES[0]), lib.render_params(W, H, 4, 1, 9))
        st = t.stats()
        before = (st.rays_traced, st.rays_answered, st.rays_cut_short, st.kernel_launches)
        assert before[0] > 0

        def others(i):
            c = cam(POSES[i])
            t.taa(synthetic_radiance(50 + i), guides(scene_name, i, jitter_of(i)), c)
            t.denoise_temporal(synthetic_radiance(60 + i), guides(scene_name, i, (0.0, 0.0)), c)

        mixed = run_sequence(t, "sliding", 0, between=others, upload=False)
        st = t.stats()
        assert before == (st.rays_traced, st.rays_answered, st.rays_cut_short, st.kernel_launches)
        for x, y in zip(alone, mixed):
            assert same_bits(x, y)


def test_a_geometry_takes_nothing_from_another_geometrys_low_pixels(tracer):
    """At rest under NO_CLAMP (the clamp box spans the 3x3 low pixels whatever their geometry; at rest the history's weights are 0 and
    1): with the low radiance of one geometry changed in every frame of a four-jitter cycle, no high pixel of another (geometry,
    bxdf) changes a bit, except where c_up fell through to the nearest low pixel, which ignores geometry."""
    scene_name = "cornell_spheres_scene"
    tracer.upload_scene(scene_of(scene_name))
    gb = guides(scene_name, 0, (0.0, 0.0))
    c = cam(POSES[0])
    g_hi = gb["ids"][..., 0]
    geoms = np.unique(g_hi[g_hi >= 0])[:3]

    def cycle(changed_geom):
        tracer.taa_upscale_reset()
        outs = []
        for call, (jx, jy) in enumerate(HALVES):
            a, b = int(2 * jx), int(2 * jy)
            ids_lo = gb["ids"][b::2, a::2]
            rad = synthetic_radiance(500 + call, *LO)
            if changed_geom is not None:
                on = ids_lo[..., 0] == changed_geom
                rad[on] = rad[on] * np.float32(3.0) + np.float32(0.25)
            outs.append(tracer.taa_upscale(rad, {"ids": ids_lo}, gb, c, lib.taa_upscale_params(flags=T.TAA_NO_CLAMP, lo_jitter=(jx, jy)))[1])
        return outs

    base = cycle(None)
    ref = TaaUpscaleRef()
    fell = []
    for call, (jx, jy) in enumerate(HALVES):
        a, b = int(2 * jx), int(2 * jy)
        r = ref.step(synthetic_radiance(500 + call, *LO), gb["ids"][b::2, a::2], gb, c, scene_models(scene_of(scene_name)),
                     lib.taa_upscale_params(flags=T.TAA_NO_CLAMP, lo_jitter=(jx, jy)))
        fell.append((r["case"] == SPATIAL) & r["fell"])
    print(f"pixels whose c_up is the nearest low pixel as it is, per call: {[int(f.sum()) for f in fell]} of {W * H}")
    for geom in geoms:
        for call, out in enumerate(cycle(int(geom))):
            others = (g_hi != geom) & ~fell[call]
            assert np.array_equal(bits(out[others]), bits(base[call][others])), (int(geom), call)
            assert not np.array_equal(bits(out[g_hi == geom]), bits(base[call][g_hi == geom]))


def test_non_finite_low_pixels_never_enter_the_history(tracer):
    scene_name = "cornell_wahoo_scene"
    tracer.upload_scene(scene_of(scene_name))
    tracer.taa_upscale_reset()
    gb = guides(scene_name, 0, (0.0, 0.0))
    c = cam(POSES[0])
    ys, xs = np.nonzero(gb["ids"][::2, ::2, 0] >= 0)
    bad_nan, bad_inf = (ys[len(ys) // 3], xs[len(ys) // 3]), (ys[2 * len(ys) // 3], xs[2 * len(ys) // 3])
    ref = TaaUpscaleRef()
    for call, (jx, jy) in enumerate(HALVES):
        a, b = int(2 * jx), int(2 * jy)
        rad = synthetic_radiance(600 + call, *LO)
        rad[bad_nan] = np.nan
        rad[bad_inf] = (1.0, np.inf, 1.0)
        p = lib.taa_upscale_params(flags=T.TAA_NO_CLAMP, lo_jitter=(jx, jy))
        _, out = tracer.taa_upscale(rad, {"ids": gb["ids"][b::2, a::2]}, gb, c, p)
        _, length = tracer.taa_upscale_history()
        r = ref.step(rad, gb["ids"][b::2, a::2], gb, c, scene_models(scene_of(scene_name)), p)
        allowed = (r["case"] == SPATIAL) & r["fell"] & ~np.isfinite(r["out"]).all(-1)  # c_up's last fallback reads a bad pixel
        print(f"call {call}: {int((~np.isfinite(out).all(-1)).sum())} non-finite outputs, {int(allowed.sum())} allowed")
        assert allowed.sum() <= 2 * 16
        assert np.isfinite(out[~allowed]).all() and np.isfinite(length).all()
    # after the cycle every output - which is the stored history - is finite
    assert np.isfinite(out).all()
    _, again = tracer.taa_upscale(rad, {"ids": gb["ids"][b::2, a::2]}, gb, c, p)  # (a call that reads the stored history)
    assert np.isfinite(again).all()


def test_repeatable_and_host_equals_device(tracer):
    import torch
    with lib.Tracer(0) as other:
        a = run_sequence(other, "sliding", 0)
    b = run_sequence(tracer, "sliding", 0)
    for x, y in zip(a, b):
        assert same_bits(x, y)
    tracer.taa_upscale_reset()
    d8 = torch.zeros((H, W, 3), dtype=torch.uint8, device="cuda")
    d_out = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")
    for i, (scene_name, k) in enumerate(SEQUENCES["sliding"]):
        j = jitter_of(i)
        hi = guides(scene_name, k, (0.0, 0.0))
        d_pos = torch.from_numpy(np.ascontiguousarray(hi["position"])).cuda()
        d_ids = torch.from_numpy(np.ascontiguousarray(hi["ids"])).cuda()
        d_ids_lo = torch.from_numpy(np.ascontiguousarray(guides(scene_name, k, j, *LO)["ids"])).cuda()
        d_rad = torch.from_numpy(synthetic_radiance(100 + i, *LO)).cuda()
        torch.cuda.synchronize()
        tracer.taa_upscale_device(cam(POSES[k]), LO[0], LO[1], d_rad.data_ptr(), d_ids_lo.data_ptr(), W, H, d_pos.data_ptr(), d_ids.data_ptr(),
                                  params_of(0, j), rgb8_ptr=d8.data_ptr(), radiance_out_ptr=d_out.data_ptr())
        assert np.array_equal(d8.cpu().numpy(), b[i][0]) and np.array_equal(bits(d_out.cpu().numpy()), bits(b[i][1])), i
    motion, length = tracer.taa_upscale_history()
    assert np.array_equal(bits(motion), bits(b[2][2])) and np.array_equal(bits(length), bits(b[2][3]))


def test_every_refused_call_names_its_field_and_leaves_the_history(tracer):
    scene_name = "cornell_wahoo_scene"
    tracer.upload_scene(scene_of(scene_name))
    tracer.taa_upscale_reset()
    gb = guides(scene_name, 0, (0.0, 0.0))
    c = cam(POSES[0])
    rad = np.ascontiguousarray(synthetic_radiance(1, *LO))
    ids_lo = np.ascontiguousarray(gb["ids"][::2, ::2])
    pos, ids = np.ascontiguousarray(gb["position"]), np.ascontiguousarray(gb["ids"])
    out = np.zeros((H, W, 3), dtype=np.float32)
    handle = lib.load()
    state = tracer._state

    def valid_call():
        tracer.taa_upscale(rad, {"ids": ids_lo}, gb, c)
        return tracer.taa_upscale_history()[1].max()

    def call(state=state, camera=c, p=None, lo=LO, hi=(W, H), rad_p=rad.ctypes.data, ids_lo_p=ids_lo.ctypes.data, pos_p=pos.ctypes.data,
             ids_p=ids.ctypes.data, no_params=False):
        p = p if p is not None else lib.taa_upscale_params()
        st = handle.ff_taa_upscale(state, C.byref(camera) if camera is not None else None, None if no_params else C.byref(p), lo[0], lo[1], rad_p,
                                   ids_lo_p, hi[0], hi[1], pos_p, ids_p, 0, None, 0, out.ctypes.data, 0)
        return st, handle.ff_last_error().decode()

    singular = cam(POSES[0])
    singular.m_forward = T.FfVec3(0.0, 0.0, 0.0)
    P = lib.taa_upscale_params
    refused = [
        (dict(state=None), "state"), (dict(camera=None), "camera"), (dict(no_params=True), "params"),
        (dict(rad_p=None), "radiance_lo"), (dict(ids_lo_p=None), "ids_lo"), (dict(pos_p=None), "position"), (dict(ids_p=None), "ids"),
        (dict(lo=(0, 45)), "lo_width"), (dict(lo=(80, 0)), "lo_height"), (dict(lo=(161, 45)), "width"), (dict(lo=(80, 91)), "height"),
        (dict(lo=(19, 45)), "width"), (dict(lo=(80, 11)), "height"), (dict(lo=(10000, 45), hi=(65536, 90)), "width"),
        (dict(lo=(80, 10000), hi=(160, 65536)), "height"),
        (dict(p=P(alpha_min=0.0)), "alpha_min"), (dict(p=P(alpha_min=1.5)), "alpha_min"), (dict(p=P(alpha_min=float("nan"))), "alpha_min"),
        (dict(p=P(gamma=0.0)), "gamma"), (dict(p=P(gamma=float("inf"))), "gamma"),
        (dict(p=P(lo_jitter=(-0.1, 0.0))), "lo_jitter"), (dict(p=P(lo_jitter=(0.0, 1.0))), "lo_jitter"),
        (dict(p=P(lo_jitter=(float("nan"), 0.0))), "lo_jitter"), (dict(p=P(lo_jitter=(0.0, float("inf")))), "lo_jitter"),
        (dict(p=P(flags=4)), "flags"), (dict(p=P(reserved=1)), "reserved"), (dict(camera=singular), "singular"),
    ]
    assert valid_call() == 1
    n = 1
    for kwargs, field in refused:
        st, message = call(**kwargs)
        assert st == T.FF_ERR_INVALID_ARG and "ff_taa_upscale" in message and field in message, (kwargs, st, message)
        n += 1
        assert valid_call() == n, (kwargs, n)  # (the history was left as it was: the lengths go on)
    with lib.Tracer(0) as empty:
        st, message = call(state=empty._state)
        assert st == T.FF_ERR_NO_SCENE and "ff_taa_upscale" in message and "scene" in message, (st, message)
        with pytest.raises(lib.FireflyError):
            empty.taa_upscale_history()


def test_jittered_half_resolution_frames_recover_a_texture_no_low_frame_carries(tracer):
    """cornell_spheres_scene with a checker of 64 squares across the back wall (1.7 high pixels a square: its period is below two
    pixels of an 80 x 45 frame), 8 bounces, NEE, at rest.  16 half-resolution frames of 16 spp under ff_jitter_sequence(i, 16) through
    ff_taa_upscale (NO_CLAMP) against the bilinear upsample of the mean of 16 unjittered half-resolution frames with the same seeds,
    both against a 1 024-spp 160 x 90 frame over the back wall's pixels.  DESIGN.md section 8 row 15 records the measured ratios."""
    nee = dict(shade_mode=T.SHADE_DIFFUSE_PATH_NEE)
    c_hi, c_lo = cam(POSES[0]), cam(POSES[0], *LO)
    with lib.Tracer(0) as t:
        t.upload_scene(scenes.cornell_spheres_scene())
        t.set_albedo_texture(BACK_WALL, t.create_texture(scenes.checker_texture(128, 128, cells=64)))
        hi = t.gbuffer(c_hi, lib.render_params(W, H))
        _, ref = t.render(c_hi, lib.render_params(W, H, 8, 1024, 77, **nee))
        mean = np.zeros((LO[1], LO[0], 3))
        for i in range(16):
            mean += t.render(c_lo, lib.render_params(*LO, 8, 16, 1000 + i, **nee))[1]
        plain = bilinear_ref(mean / 16, H, W)
        results = {}
        for name, flags in (("no clamp", T.TAA_NO_CLAMP), ("clamped", 0)):
            t.taa_upscale_reset()
            for i in range(16):
                j = jitter_of(i)
                t.set_pixel_jitter(*j)
                _, frame = t.render(c_lo, lib.render_params(*LO, 8, 16, 1000 + i, **nee))
                lo = t.gbuffer(c_lo, lib.render_params(*LO))
                t.set_pixel_jitter(0.0, 0.0)
                _, results[name] = t.taa_upscale(frame, lo, hi, c_hi, lib.taa_upscale_params(flags=flags, lo_jitter=j))
    wall = hi["ids"][..., 0] == BACK_WALL
    assert wall.sum() > 1000
    mse = lambda a, m: float(np.mean((np.asarray(a, np.float64)[m] - ref[m]) ** 2))  # noqa: E731
    everywhere = np.ones((H, W), bool)
    temporal, bilinear = mse(results["no clamp"], wall), mse(plain, wall)
    print(f"back wall: MSE temporal {temporal:.4g}, bilinear {bilinear:.4g}, ratio {temporal / bilinear:.3f}; clamped ratio "
          f"{mse(results['clamped'], wall) / bilinear:.3f}; whole frame ratio {mse(results['no clamp'], everywhere) / mse(plain, everywhere):.3f} "
          f"(clamped {mse(results['clamped'], everywhere) / mse(plain, everywhere):.3f})")
    assert temporal < bilinear, (temporal, bilinear)
