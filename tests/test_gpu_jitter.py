"""Sub-pixel jitter on the GPU (ff_set_pixel_jitter): the jittered G-buffer bit for bit against the CPU oracle's intersectRays of
each pixel's ray through ff_camera_ray_matrix_jittered, the NORMAL_DEBUG frame against it, jitter 0 0 leaving every frame as it
was, the stored primary hits re-keyed by a new jitter, and the partitions of a jittered frame."""
import ctypes as C
import functools

import numpy as np
import pytest

from gpupathtracer_amd import lib, scenes
from gpupathtracer_amd import types as T
from gbuffer_ref import surface_colour
from oracle_lib import load_oracle

pytestmark = pytest.mark.gpu

W, H = 96, 54
JITTERS = [(0.5, 0.25), (0.999, 0.5), (0.125, 0.875)]


def c2(w=W, h=H):
    return scenes.posed_camera(w, h, position=(0.0, 0.0, 2.4), yaw=-90.0, pitch=0.0)


def oblique(w=W, h=H):
    return scenes.posed_camera(w, h, position=(7.0, 3.0, 9.0), yaw=-128.0, pitch=-14.0)


POSES = {"c2": (scenes.cornell_wahoo_scene, c2), "oblique": (scenes.blooper_scene, oblique)}


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@functools.lru_cache(maxsize=None)
def scene_of(pose):
    return POSES[pose][0]()


def oracle_gbuffer_jittered(scene, camera, params, jx, jy):
    """gbuffer_ref.oracle_gbuffer with ff_camera_ray_matrix_jittered(camera, jx, jy) as the ray matrix."""
    lib_o = load_oracle()
    mat = (C.c_float * 16)(*lib.camera_ray_matrix_jittered(camera, jx, jy).m[:])
    out = {"depth": np.zeros((H, W), np.float32), "position": np.zeros((H, W, 3), np.float32), "normal": np.zeros((H, W, 3), np.float32),
           "albedo": np.zeros((H, W, 3), np.float32), "ids": np.full((H, W, 3), -1, np.int32)}
    colours = [surface_colour(scene.geometries[i]) for i in range(len(scene))]
    ray, isect = T.FfRay(), T.FfIntersect()
    for y in range(params.height):
        for x in range(params.width):
            lib_o.orc_primary_ray(mat, C.byref(camera), x, y, C.byref(ray))
            lib_o.orc_intersect_rays(C.byref(ray), scene.geometries, len(scene), C.byref(isect))
            if not isect.m_hit:
                continue
            out["depth"][y, x] = isect.m_t
            out["position"][y, x] = isect.m_intersectionPoint.tuple()
            out["normal"][y, x] = isect.m_normal.tuple()
            col, kind = colours[isect.geometryIndex]
            out["albedo"][y, x] = col
            out["ids"][y, x] = (isect.geometryIndex, isect.triangleIndex, kind)
    return out


@functools.lru_cache(maxsize=None)
def oracle_case(pose, jitter):
    cam = POSES[pose][1]()
    return oracle_gbuffer_jittered(scene_of(pose), cam, lib.render_params(W, H), *jitter)


@pytest.mark.parametrize("jitter", JITTERS)
@pytest.mark.parametrize("pose", sorted(POSES))
def test_jittered_g_buffer_and_normal_frame_match_the_oracle(tracer, pose, jitter):
    cam = POSES[pose][1]()
    want = oracle_case(pose, jitter)
    tracer.upload_scene(scene_of(pose))
    tracer.set_pixel_jitter(*jitter)
    try:
        for mode in (T.TRACE_BVH, T.TRACE_BRUTE_FORCE):
            got = tracer.gbuffer(cam, lib.render_params(W, H, trace_mode=mode))
            for k in want:
                bad = np.argwhere(bits(got[k]) != bits(want[k]))
                assert bad.size == 0, f"{pose} {jitter} mode {mode} {k}: {len(bad)} differ, first {bad[:3].tolist()}"
            # NORMAL_DEBUG (kernel.cu shade(), ff_k_shade.h settle_hit): |normal| per channel, misses 0
            _, rad = tracer.render(cam, lib.render_params(W, H, 1, 1, 3, trace_mode=mode, shade_mode=T.SHADE_NORMAL_DEBUG))
            hit = want["ids"][..., 0] >= 0
            expect = np.where(hit[..., None], np.abs(want["normal"]), np.float32(0))
            assert np.array_equal(bits(rad), bits(expect)), (pose, jitter, mode)
        # the jitter does move the rays
        unjittered = oracle_case(pose, (0.0, 0.0))
        assert not np.array_equal(bits(unjittered["depth"]), bits(want["depth"]))
    finally:
        tracer.set_pixel_jitter(0.0, 0.0)


def frames_of(t, cam, every_mode=True):
    out = []
    modes = (T.SHADE_NORMAL_DEBUG, T.SHADE_DIFFUSE_PATH, T.SHADE_DIFFUSE_PATH_SMOOTH) if every_mode else (T.SHADE_DIFFUSE_PATH,)
    for shade in modes:
        for spp in (1, 4):
            rgb8, rad = t.render(cam, lib.render_params(W, H, 6, spp, 21, shade_mode=shade))
            out.append((rgb8, bits(rad).copy()))
    gb = t.gbuffer(cam, lib.render_params(W, H))
    out += [(None, bits(gb[k]).copy()) for k in sorted(gb)]
    for f in range(3):
        rgb8, rad = t.render_progressive(cam, lib.render_params(W, H, 6, 1, 31), f)
        out.append((rgb8, bits(rad).copy()))
    return out


def test_zero_jitter_leaves_every_frame_as_it_was():
    scene, cam = scenes.cornell_wahoo_scene(), c2()
    with lib.Tracer(0) as never:
        never.upload_scene(scene)
        want = frames_of(never, cam)
    with lib.Tracer(0) as t:
        t.upload_scene(scene)
        t.set_pixel_jitter(0.0, 0.0)
        explicit = frames_of(t, cam)
        t.set_pixel_jitter(0.7, 0.2)
        t.render(cam, lib.render_params(W, H, 6, 1, 5))
        t.set_pixel_jitter(0.0, 0.0)
        back = frames_of(t, cam)
    for got in (explicit, back):
        for (a8, a), (b8, b) in zip(got, want):
            assert (a8 is None and b8 is None) or np.array_equal(a8, b8)
            assert np.array_equal(a, b)


def test_new_jitter_at_rest_re_keys_the_stored_hits():
    """At rest, a sequence that changes the jitter between 1-spp and 64-spp frames: every frame is bit for bit the same frame on a
    fresh state with that jitter; so is the count of rays answered from stored hits whenever the jitter has just changed (a stale
    stored hit would answer the wrong primary ray).  Frames at rest with an unchanged jitter keep their hits, as without jitter."""
    scene, cam = scenes.cornell_wahoo_scene(), c2()
    seq = [((0.5, 0.25), 1), ((0.5, 0.25), 1), ((0.5, 0.25), 64), ((0.75, 0.125), 1), ((0.75, 0.125), 1), ((0.25, 0.625), 64),
           ((0.25, 0.625), 1), ((0.0, 0.0), 1), ((0.0, 0.0), 64), ((0.5, 0.25), 1)]
    with lib.Tracer(0) as t:
        t.upload_scene(scene)
        t.set_collect_stats(True)
        for k, (j, spp) in enumerate(seq):
            t.set_pixel_jitter(*j)
            params = lib.render_params(W, H, 6, spp, 100 + k)
            rgb8, rad = t.render(cam, params)
            answered = t.stats().rays_answered
            gb = t.gbuffer(cam, lib.render_params(W, H))
            with lib.Tracer(0) as fresh:
                fresh.upload_scene(scene)
                fresh.set_collect_stats(True)
                fresh.set_pixel_jitter(*j)
                f8, frad = fresh.render(cam, params)
                f_answered = fresh.stats().rays_answered
                fgb = fresh.gbuffer(cam, lib.render_params(W, H))
            assert np.array_equal(rgb8, f8) and np.array_equal(bits(rad), bits(frad)), (k, j, spp)
            if k > 0 and j != seq[k - 1][0]:  # a new jitter answers nothing from the hits stored for the old one
                assert answered == f_answered, (k, answered, f_answered)
            assert all(np.array_equal(bits(gb[n]), bits(fgb[n])) for n in gb), k


def test_jittered_partitions_and_brute_force_agree(tracer):
    tracer.upload_scene(scenes.cornell_wahoo_scene())
    cam = c2()
    tracer.set_pixel_jitter(0.999, 0.5)
    try:
        params = lib.render_params(W, H, 6, 2, 9)
        w8, whole = tracer.render(cam, params)
        b8, brute = tracer.render(cam, lib.render_params(W, H, 6, 2, 9, trace_mode=T.TRACE_BRUTE_FORCE))
        assert np.array_equal(w8, b8) and np.array_equal(bits(whole), bits(brute))
        # strips of 8 rows over 3 parts: part p owns strips s with s % 3 == p, compacted in increasing s
        strip_rows, parts = 8, 3
        rows = np.arange(H)
        for p in range(parts):
            mine = rows[(rows // strip_rows) % parts == p]
            s8, srad = tracer.render_strips(cam, params, strip_rows, p, parts)
            assert srad.shape[0] == len(mine)
            assert np.array_equal(s8, w8[mine]) and np.array_equal(bits(srad), bits(whole[mine])), p
        for x0, y0, tw, th in ((0, 0, 32, 16), (37, 11, 40, 30), (W - 9, H - 5, 9, 5)):
            t8, trad = tracer.render_tile(cam, params, x0, y0, tw, th)
            assert np.array_equal(t8, w8[y0:y0 + th, x0:x0 + tw]) and np.array_equal(bits(trad), bits(whole[y0:y0 + th, x0:x0 + tw]))
    finally:
        tracer.set_pixel_jitter(0.0, 0.0)
