"""Multi-bounce paths of nee_path_kernel, sample by sample, against the float64 walker (tests/path_ref.py): both path modes at depth
under a light table, an environment, textures, rough mirrors, camera sampling and a pixel jitter.  Every case is a handful of 32x24
frames; the walker traces its rays through ff_intersect_rays of the same tracer.

The rule (path_ref.py states where its tolerance comes from): non-excused hit pixels are within |got - ref| <= 1e-4 |ref| + 1e-6, at
least 99.5 % of the hit pixels are within it, at most 10 % are excused, and the walker's counter of the branch a case exists for is
positive over the case's frames."""
import numpy as np
import pytest

from gpupathtracer_amd import lib, scenes
from gpupathtracer_amd import types as T
import env_ref
import glossy_ref
import nee_ref
import path_ref
from test_gpu_camera import MIRROR_BACK, MIRROR_CUBE, MIRROR_FLOOR

pytestmark = pytest.mark.gpu

NEE, PATH = T.SHADE_DIFFUSE_PATH_NEE, T.SHADE_DIFFUSE_PATH
W, H = 32, 24
INSIDE = dict(position=(0.0, 0.0, 2.4), yaw=-90.0, pitch=0.0)
GRAZING = dict(position=(0.0, -2.3, 2.4), yaw=-90.0, pitch=-2.0)  # just above the floor, looking along it
FRAMES = ((1, 1), (1, 2), (1, 3), (3, 4))  # (spp, seed): single samples, and three of a pixel (the sample bits, the reset between samples)
EXCUSE_CAP = 0.10


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---- scenes and bindings --------------------------------------------------------------------------------------------------------------

def bright_texel_map(floor=0.2, value=30.0):
    """8x4, one bright texel: with ROTATION it covers the directions out of the box's open front, above the horizon."""
    env = np.full((4, 8, 3), floor, np.float32)
    env[1, 3] = (value, 0.9 * value, 0.7 * value)
    return env


ROTATION = 20.0
TEXELS = np.random.default_rng(11).uniform(0.2, 1.0, (4, 4, 3)).astype(np.float32)  # a 4x4 checker of distinct texels
TEX_MESH, TEX_FLOOR, TEX_SPHERE = 0, 2, 6
SPHERES_FLOOR, SPHERES_MIRROR = 2, 9  # cornell_spheres_scene: the floor plane (made a mirror below) and the mirror sphere


def textured_scene():
    """The open-front box with a cube mesh, a sphere and an emitter plane under the ceiling; the cube, the floor and the sphere take
    the texture."""
    s = scenes.Scene()
    s.add_mesh(scenes.load_mesh("cube"), (0.9, -2.0, -0.5), (0, 25, 0), (1, 1, 1), scenes.make_bxdf(T.BXDF_DIFFUSE, albedo=(0.8, 0.7, 0.6)))
    nee_ref._box_planes(s)
    s.add_sphere(0.7, (-1.0, -1.8, 0.2), (0, 30, 0), (1, 1, 1), scenes.make_bxdf(T.BXDF_DIFFUSE, albedo=(0.9, 0.9, 0.5)))
    s.add_plane((0, 2.49, 0), (90, 0, 0), (2, 2, 2), scenes.make_bxdf(T.BXDF_EMITTER, emissive=(1, 1, 1), intensity=2.0))
    return s.finalize()


TEXTURES = {TEX_MESH: (TEXELS, 0, (1.0, 1.0), (0.0, 0.0)), TEX_FLOOR: (TEXELS, 0, (3.0, 2.0), (0.1, 0.2)), TEX_SPHERE: (TEXELS, 0, (2.0, 1.0), (0.0, 0.0))}


def rough_scene():
    """cornell_spheres_scene with its floor made a mirror: a plane and a sphere to bind a roughness to."""
    return glossy_ref.with_mirror(scenes.cornell_spheres_scene(), SPHERES_FLOOR)


def everything():
    """test_gpu_camera.py's bind_everything and the setting of its `loaded` fixture."""
    env = np.full((8, 16, 3), 0.3, np.float32)
    env[2, 5] = (40.0, 36.0, 28.0)
    texels = np.random.default_rng(2).uniform(0.2, 1.0, (8, 8, 3)).astype(np.float32)
    return dict(scene=scenes.cornell_mirror_scene(), environment=(env, 1.0, 20.0), textures={MIRROR_FLOOR: (texels, 0, (3.0, 2.0), (0.0, 0.0))},
                roughness={MIRROR_CUBE: 0.3, MIRROR_BACK: 0.2}, sampling=lib.camera_sampling(T.PIXEL_BOX, 0.08, 2.5))


def case(scene, mode, bounces, counters=(), pose=INSIDE, brute=False, frames=FRAMES, **bound):
    return dict(scene=scene, mode=mode, bounces=bounces, counters=counters, pose=pose, brute=brute, frames=frames, **bound)


DEEP = ("light_samples_deep", "mis_emitter_hits_deep")
CASES = {
    # diffuse depth: prev_pdf from vertex to vertex, the segment index in the three streams, beta at a deep light sample
    "diffuse_b1": lambda: case(nee_ref.triangle_light_scene(), NEE, 1),  # (emitters only, no light sample)
    "diffuse_b3": lambda: case(nee_ref.triangle_light_scene(), NEE, 3, DEEP, brute=True),
    "diffuse_b5": lambda: case(nee_ref.triangle_light_scene(), NEE, 5, DEEP),
    "diffuse_b3_jitter": lambda: case(nee_ref.triangle_light_scene(), NEE, 3, DEEP, jitter=(0.3, 0.8)),  # (ff_set_pixel_jitter takes [0, 1): 0.8 is -0.2 of the next pixel)
    # specular chains: weight 1 after mirror or glass, light samples at vertices reached through them, refracted origins
    "mirror_b5": lambda: case(scenes.cornell_mirror_scene(), NEE, 5, ("light_samples_deep", "emitter_hits_after_specular"), brute=True),
    "glass_b5": lambda: case(scenes.cornell_glass_scene(), NEE, 5, ("light_samples_deep", "emitter_hits_after_specular", "refracted_segments")),
    "spheres_b5": lambda: case(scenes.cornell_spheres_scene(), NEE, 5, DEEP),
    "sphere_light_b5": lambda: case(nee_ref.sphere_light_scene(), NEE, 5),  # (an emitter outside the table: every weight 1)
    # the environment: (a) with the light table, (b) alone; in the path mode the NEE kernel runs with no light table
    "env_table_nee": lambda: case(nee_ref.triangle_light_scene(), NEE, 4, DEEP + ("env_misses_last_segment",), brute=True,
                                  environment=(bright_texel_map(), 1.5, ROTATION)),
    "env_alone_nee": lambda: case(nee_ref.triangle_light_scene(0.0), NEE, 4, ("light_samples_deep", "env_misses_last_segment"),
                                  environment=(bright_texel_map(), 1.5, ROTATION)),
    "env_table_path": lambda: case(nee_ref.triangle_light_scene(), PATH, 4, ("env_misses_last_segment",), environment=(bright_texel_map(), 1.5, ROTATION)),
    "env_alone_path": lambda: case(nee_ref.triangle_light_scene(0.0), PATH, 4, ("env_misses_last_segment",), environment=(bright_texel_map(), 1.5, ROTATION)),
    # textures at hits that are not the primary hit (no environment: the path mode goes through TEX = 1 as well)
    "textures_nee": lambda: case(textured_scene(), NEE, 4, ("texture_lookups_deep", "light_samples_deep"), brute=True, textures=TEXTURES),
    "textures_path": lambda: case(textured_scene(), PATH, 4, ("texture_lookups_deep",), textures=TEXTURES),
    # rough mirrors on a plane and a sphere
    "rough_0.05_nee": lambda: case(rough_scene(), NEE, 4, DEEP, brute=True, roughness={SPHERES_FLOOR: 0.05, SPHERES_MIRROR: 0.05}),
    "rough_0.6_nee": lambda: case(rough_scene(), NEE, 4, DEEP, roughness={SPHERES_FLOOR: 0.6, SPHERES_MIRROR: 0.6}),
    "rough_0.05_path": lambda: case(rough_scene(), PATH, 4, roughness={SPHERES_FLOOR: 0.05, SPHERES_MIRROR: 0.05}),
    "rough_0.6_path": lambda: case(rough_scene(), PATH, 4, roughness={SPHERES_FLOOR: 0.6, SPHERES_MIRROR: 0.6}),
    "rough_grazing": lambda: case(rough_scene(), NEE, 4, ("glossy_deaths_pending_shadow",), pose=GRAZING, roughness={SPHERES_FLOOR: 0.6, SPHERES_MIRROR: 0.6}),
    # lens, box filter, environment, texture and rough mirrors at once
    "everything": lambda: case(mode=NEE, bounces=4, counters=("light_samples_deep", "texture_lookups_deep", "env_misses_last_segment"), brute=True,
                               frames=((3, 4), (1, 1)), **everything()),
}


_TEXTURES = []  # ids of the textures bind() made for the running test


@pytest.fixture
def pt(tracer):
    """The session's tracer, with no environment, today's camera and no jitter before and after; textures made through it are destroyed."""
    def reset():
        tracer.set_camera_sampling(None)
        tracer.set_pixel_jitter(0.0, 0.0)
        tracer.clear_environment()

    reset()
    yield tracer
    while _TEXTURES:
        tracer.destroy_texture(_TEXTURES.pop())
    reset()


def bind(t, cfg):
    """The case's scene and bindings on the tracer."""
    t.upload_scene(cfg["scene"])
    if cfg.get("environment") is not None:
        t.set_environment(*cfg["environment"])
    else:
        t.clear_environment()
    for g, (texels, flags, scale, offset) in (cfg.get("textures") or {}).items():
        _TEXTURES.append(t.create_texture(texels, flags))
        t.set_albedo_texture(g, _TEXTURES[-1], scale, offset)
    for g, r in (cfg.get("roughness") or {}).items():
        t.set_roughness(g, r)
    t.set_camera_sampling(cfg.get("sampling"))
    t.set_pixel_jitter(*cfg.get("jitter", (0.0, 0.0)))


def walk(t, cfg, camera, params):
    return path_ref.walk(t.intersect_rays, cfg["scene"], camera, params, environment=cfg.get("environment"), textures=cfg.get("textures"),
                         roughness=cfg.get("roughness"), sampling=cfg.get("sampling"), jitter=cfg.get("jitter", (0.0, 0.0)))


def check_frame(got, ref, excused, hit, label):
    ok = path_ref.within(got, ref)
    bad = hit & ~ok & ~excused
    worst = (np.abs(got - ref) / (path_ref.RTOL * np.abs(ref) + path_ref.ATOL))[hit & ~excused].max() if (hit & ~excused).any() else 0.0
    print(f"{label}: {ok[hit].mean():.5f} of {hit.sum()} hit pixels within tolerance, {excused[hit].mean():.5f} excused, {bad.sum()} off and unexcused, "
          f"largest deviation {worst:.3f} of the allowance")
    assert not bad.any(), f"{label}: {bad.sum()} pixels off the walker that no ray decision excuses: {np.argwhere(bad)[:5]}, got {got[bad][:3]}, ref {ref[bad][:3]}"
    assert ok[hit].mean() >= 0.995, f"{label}: {ok[hit].mean():.4f} of hit pixels within tolerance"
    assert excused[hit].mean() <= EXCUSE_CAP, f"{label}: {excused[hit].mean():.4f} of hit pixels excused"


@pytest.mark.parametrize("name", sorted(CASES))
def test_paths_match_the_walker(pt, name):
    cfg = CASES[name]()
    c = scenes.posed_camera(W, H, **cfg["pose"])
    bind(pt, cfg)
    total = {k: 0 for k in path_ref.COUNTERS}
    lit = False
    for spp, seed in cfg["frames"]:
        p = lib.render_params(W, H, cfg["bounces"], spp, seed=seed, trace_mode=T.TRACE_BVH, shade_mode=cfg["mode"])
        got = pt.render(c, p)[1]
        ref, excused, stats = walk(pt, cfg, c, p)
        hit = stats["hit"]
        assert hit.sum() > 0.5 * W * H
        check_frame(got.astype(np.float64), ref, excused, hit, f"{name} spp {spp} seed {seed}")
        if cfg.get("environment") is None:
            assert np.all(got[~hit] == 0.0)
        lit = lit or ref[hit].max() > 0.0
        for k in total:
            total[k] += stats[k]
        if cfg["brute"]:  # (the same frame from the other traversal: the reference is shared)
            p.trace_mode = T.TRACE_BRUTE_FORCE
            check_frame(pt.render(c, p)[1].astype(np.float64), ref, excused, hit, f"{name} spp {spp} seed {seed} brute force")
    print(name, total)
    assert lit
    for k in cfg["counters"]:
        assert total[k] > 0, f"{name} never reached its branch: {k} = 0"


# ---- an all-zero map at depth ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", [NEE, PATH])
def test_black_environment_is_no_environment_at_depth(pt, mode):
    scene = nee_ref.triangle_light_scene()
    c = scenes.posed_camera(W, H, **INSIDE)
    pt.upload_scene(scene)
    for spp, seed in FRAMES:
        p = lib.render_params(W, H, 4, spp, seed=seed, shade_mode=mode)
        pt.clear_environment()
        want = pt.render(c, p)
        pt.set_environment(np.zeros((4, 8, 3), np.float32), 1.5, ROTATION)
        got = pt.render(c, p)
        assert want[1].max() > 0.0
        assert np.array_equal(bits(got[1]), bits(want[1])) and np.array_equal(got[0], want[0])
    # and the walker, which treats such a map as an environment whose table is empty, agrees with the frame
    cfg = case(scene, mode, 4, environment=(np.zeros((4, 8, 3), np.float32), 1.5, ROTATION))
    ref, excused, stats = walk(pt, cfg, c, p)
    check_frame(got[1].astype(np.float64), ref, excused, stats["hit"], "black map")


# ---- the walker at bounces = 2 is the existing references -------------------------------------------------------------------------------

def agree(a, b, hit):
    assert hit.sum() > 0.25 * W * H and np.abs(b[hit]).max() > 0.0
    assert np.abs(a - b)[hit].max() <= 1e-9, np.abs(a - b)[hit].max()


def test_walker_equals_nee_ref_at_two_bounces(pt):
    scene = nee_ref.triangle_light_scene()
    c = scenes.posed_camera(W, H, **INSIDE)
    p = lib.render_params(W, H, 2, 3, seed=2024, shade_mode=NEE)
    cfg = case(scene, NEE, 2)
    bind(pt, cfg)
    ref, hit, _ = nee_ref.direct_lighting(pt, scene, c, p)
    agree(walk(pt, cfg, c, p)[0], ref, hit)


@pytest.mark.parametrize("area_light", [False, True])
def test_walker_equals_env_ref_at_two_bounces(pt, area_light):
    scene = scenes.open_floor_scene(area_light=area_light)
    c = scenes.posed_camera(W, H, position=(0.0, -1.2, 3.0), yaw=-90.0, pitch=0.0)  # test_gpu_env.py's OPEN pose
    p = lib.render_params(W, H, 2, 3, seed=2024, shade_mode=NEE)
    sky = scenes.sun_sky_map(64, 32)
    cfg = case(scene, NEE, 2, environment=(sky, 0.5, 30.0))
    bind(pt, cfg)
    ref, hit, _ = env_ref.direct_lighting(pt, scene, c, p, sky, 0.5, 30.0)
    agree(walk(pt, cfg, c, p)[0], ref, hit)


def test_walker_equals_glossy_ref_at_two_bounces(pt):
    back = 2  # triangle_light_scene's back wall, as test_gpu_glossy.py binds it
    scene = glossy_ref.with_mirror(nee_ref.triangle_light_scene(), back)
    c = scenes.posed_camera(W, H, **INSIDE)
    p = lib.render_params(W, H, 2, 3, seed=2024, shade_mode=NEE)
    cfg = case(scene, NEE, 2, roughness={back: 0.3})
    bind(pt, cfg)
    ref, hit, _ = glossy_ref.direct_lighting(pt, scene, c, p, {back: 0.3})
    agree(walk(pt, cfg, c, p)[0], ref, hit)


def test_walker_equals_glossy_ref_under_an_environment(pt):
    scene = glossy_ref.sphere_on_floor_scene()
    c = scenes.posed_camera(W, H, position=(0.0, 0.6, 4.0), yaw=-90.0, pitch=-8.0)  # test_gpu_glossy.py's OUTSIDE pose
    p = lib.render_params(W, H, 2, 3, seed=77, shade_mode=NEE)
    env = np.zeros((8, 16, 3), np.float32)
    env[2, 5] = (400.0, 360.0, 280.0)
    cfg = case(scene, NEE, 2, environment=(env, 1.0, 20.0), roughness={0: 0.3})
    bind(pt, cfg)
    ref, hit, _ = glossy_ref.direct_lighting(pt, scene, c, p, {0: 0.3}, env=(env, 1.0, 20.0))
    agree(walk(pt, cfg, c, p)[0], ref, hit)
