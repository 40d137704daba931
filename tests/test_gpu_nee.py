"""FF_SHADE_DIFFUSE_PATH_NEE on the GPU: bit-identity with FF_SHADE_DIFFUSE_PATH when the light table is empty, direct lighting
against the float64 reference (tests/nee_ref.py), agreement in expectation with FF_SHADE_DIFFUSE_PATH on six scenes, determinism
across trace modes, launches, tiles, strips and progressive frames, emission scaling, dynamic scenes, isolation from the other
shade modes and ff_gbuffer, the variance it saves on C2, and the entry points that refuse it."""
import numpy as np
import pytest

from gpupathtracer_amd import lib, scenes
from gpupathtracer_amd import types as T
import nee_ref

pytestmark = pytest.mark.gpu

NEE, PATH = T.SHADE_DIFFUSE_PATH_NEE, T.SHADE_DIFFUSE_PATH
INSIDE = dict(position=(0.0, 0.0, 2.4), yaw=-90.0, pitch=0.0)


def cam(w, h, **pose):
    return scenes.posed_camera(w, h, **(pose or INSIDE))


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def render(tracer, scene, camera, params):
    tracer.upload_scene(scene)
    return tracer.render(camera, params)[1]


# ---- an empty light table is FF_SHADE_DIFFUSE_PATH bit for bit ------------------------------------------------------------

@pytest.fixture(scope="module")
def sphere_light():
    return nee_ref.sphere_light_scene()


@pytest.mark.parametrize("trace", [T.TRACE_BVH, T.TRACE_BRUTE_FORCE])
@pytest.mark.parametrize("bounces", [1, 3, 8])
@pytest.mark.parametrize("spp", [1, 5, 130, 1100])
@pytest.mark.parametrize("jitter", [False, True])
def test_empty_table_is_the_path_mode_bit_for_bit(tracer, sphere_light, trace, bounces, spp, jitter):
    if trace == T.TRACE_BRUTE_FORCE and spp > 130:
        spp = 130 + bounces  # (brute force: the same code paths at a tenth of the cost)
    w, h = 24, 16
    assert len(lib.light_table(sphere_light)[0]["area"]) == 0
    tracer.upload_scene(sphere_light)
    tracer.set_pixel_jitter(*(lib.jitter_sequence(3) if jitter else (0.0, 0.0)))
    try:
        c = cam(w, h)
        a = tracer.render(c, lib.render_params(w, h, bounces, spp, seed=11, trace_mode=trace, shade_mode=PATH))
        b = tracer.render(c, lib.render_params(w, h, bounces, spp, seed=11, trace_mode=trace, shade_mode=NEE))
    finally:
        tracer.set_pixel_jitter(0.0, 0.0)
    assert np.array_equal(bits(a[1]), bits(b[1]))
    assert np.array_equal(a[0], b[0])
    assert a[1].max() > 0.0 or bounces == 1  # (one segment: only pixels that see the sphere itself are lit)


# ---- direct lighting against the float64 reference ------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["C2", "triangle_lights"])
@pytest.mark.parametrize("spp", [1, 2, 4])
def test_direct_lighting_matches_the_reference(tracer, name, spp):
    scene = scenes.cornell_wahoo_scene() if name == "C2" else nee_ref.triangle_light_scene()
    w, h = 96, 64
    c = cam(w, h)
    params = lib.render_params(w, h, bounces=2, spp=spp, seed=2024, shade_mode=NEE)
    got = render(tracer, scene, c, params).astype(np.float64)
    ref, hit, excused = nee_ref.direct_lighting(tracer, scene, c, params)
    ok = np.all(np.abs(got - ref) <= 1e-4 * np.abs(ref) + 1e-6, -1)
    frac = ok[hit].mean()
    # rule: a pixel is excused when one of its shadow or BSDF rays changes its answer under a turn of 2e-5 rad (nee_ref)
    assert frac >= 0.995, f"{frac:.4f} of hit pixels within tolerance"
    bad = hit & ~ok & ~excused
    assert not bad.any(), f"{bad.sum()} pixels off the reference that no ray decision excuses: {np.argwhere(bad)[:5]}"
    assert excused[hit].mean() <= 0.05
    assert (ref[hit] > 0).any()


# ---- same expectation as FF_SHADE_DIFFUSE_PATH -----------------------------------------------------------------------------

UNBIASED_SCENES = {
    "C2": scenes.cornell_wahoo_scene,
    "C3": scenes.blooper_scene,
    "mirror": scenes.cornell_mirror_scene,
    "glass": scenes.cornell_glass_scene,
    "spheres": scenes.cornell_spheres_scene,
    "triangle_lights": nee_ref.triangle_light_scene,
}


@pytest.mark.parametrize("name", sorted(UNBIASED_SCENES))
def test_same_expectation_as_the_path_mode(tracer, name):
    scene = UNBIASED_SCENES[name]()
    w, h, seeds = 48, 32, 16
    pose = dict(position=(0.0, 0.0, 9.0), yaw=-90.0, pitch=0.0) if name == "C3" else INSIDE
    c = cam(w, h, **pose)
    tracer.upload_scene(scene)
    imgs = {}
    for mode in (PATH, NEE):
        imgs[mode] = np.stack([tracer.render(c, lib.render_params(w, h, 8, 32, seed=1000 + s, shade_mode=mode))[1] for s in range(seeds)]).astype(np.float64)
    assert imgs[PATH].mean() > 0.0

    def blocks(x):  # [seed, H/8, W/8, 3] means of 8x8 blocks
        return x.reshape(seeds, h // 8, 8, w // 8, 8, 3).mean(axis=(2, 4))

    a, b = blocks(imgs[PATH]), blocks(imgs[NEE])
    se = np.sqrt(a.var(0, ddof=1) / seeds + b.var(0, ddof=1) / seeds) + 1e-7
    z = np.abs(a.mean(0) - b.mean(0)) / se
    assert z.max() < 5.0, f"block mean off by {z.max():.2f} standard errors"
    ia, ib = imgs[PATH].mean(axis=(1, 2, 3)), imgs[NEE].mean(axis=(1, 2, 3))
    zi = abs(ia.mean() - ib.mean()) / np.sqrt(ia.var(ddof=1) / seeds + ib.var(ddof=1) / seeds)
    assert zi < 4.0, f"image mean off by {zi:.2f} standard errors"


# ---- determinism ------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def tri_scene():
    return nee_ref.triangle_light_scene()


def test_repeatable_and_bvh_equals_brute_force(tracer, tri_scene):
    w, h = 40, 30
    c = cam(w, h)
    tracer.upload_scene(tri_scene)
    p = lib.render_params(w, h, 5, 9, seed=5, shade_mode=NEE)
    a = tracer.render(c, p)[1]
    b = tracer.render(c, p)[1]
    assert np.array_equal(bits(a), bits(b))
    p.trace_mode = T.TRACE_BRUTE_FORCE
    assert np.array_equal(bits(a), bits(tracer.render(c, p)[1]))


def test_independent_of_spp_per_launch(tracer, tri_scene):
    w, h = 32, 24
    c = cam(w, h)
    tracer.upload_scene(tri_scene)
    ref = tracer.render(c, lib.render_params(w, h, 4, 200, seed=8, shade_mode=NEE))[1]
    for spl in (1, 64, 128):
        got = tracer.render(c, lib.render_params(w, h, 4, 200, seed=8, shade_mode=NEE, spp_per_launch=spl))[1]
        assert np.array_equal(bits(ref), bits(got)), spl
    assert tracer.stats().kernel_launches == 2


def test_tiles_and_strips_match_the_full_frame(tracer, tri_scene):
    w, h = 44, 30
    c = cam(w, h)
    tracer.upload_scene(tri_scene)
    p = lib.render_params(w, h, 4, 3, seed=21, shade_mode=NEE)
    full = tracer.render(c, p)[1]
    for (x0, y0, tw, th) in ((0, 0, 16, 8), (13, 7, 20, 17), (40, 25, 4, 5)):
        tile = tracer.render_tile(c, p, x0, y0, tw, th)[1]
        assert np.array_equal(bits(tile), bits(full[y0:y0 + th, x0:x0 + tw])), (x0, y0)
    strip_rows, parts = 4, 3
    for part in range(parts):
        _, srad = tracer.render_strips(c, p, strip_rows, part, parts)
        rows = [y for y in range(h) if (y // strip_rows) % parts == part]
        assert np.array_equal(bits(srad), bits(full[rows])), part


def test_progressive_is_the_mean_of_its_frames(tracer, tri_scene):
    w, h = 32, 24
    c = cam(w, h)
    tracer.upload_scene(tri_scene)
    frames, acc = [], None
    for i in range(4):
        frames.append(tracer.render(c, lib.render_params(w, h, 4, 2, seed=300 + i, shade_mode=NEE))[1])
        _, mean = tracer.render_progressive(c, lib.render_params(w, h, 4, 2, seed=300, shade_mode=NEE), i)  # (frame i: seed + i)
        acc = frames[0].copy() if i == 0 else acc + frames[i]
        assert np.array_equal(bits(mean), bits(acc * np.float32(1.0 / (i + 1))))


def test_emission_scales_exactly(tracer):
    w, h = 32, 24
    c = cam(w, h)
    p = lib.render_params(w, h, 6, 4, seed=4, shade_mode=NEE)
    one = render(tracer, nee_ref.triangle_light_scene(1.0), c, p)
    two = render(tracer, nee_ref.triangle_light_scene(2.0), c, p)
    assert one.max() > 0.0
    assert np.array_equal(bits(two), bits(one * np.float32(2.0)))


# ---- dynamic scenes ---------------------------------------------------------------------------------------------------------

LIGHT_MESH = 6  # the emitting cube of nee_ref.triangle_light_scene


def test_moved_light_equals_a_fresh_upload(tracer):
    w, h = 32, 24
    c = cam(w, h)
    p = lib.render_params(w, h, 4, 4, seed=9, shade_mode=NEE)
    scene = nee_ref.triangle_light_scene()
    tracer.upload_scene(scene)
    tracer.render(c, p)
    moved = scenes.Scene()
    moved._specs = list(scene._specs)
    kind, pos, rot, scl, tris, bxdf = moved._specs[LIGHT_MESH]
    moved._specs[LIGHT_MESH] = (kind, (0.5, 1.6, -0.4), (0, 75, 10), scl, tris, bxdf)
    moved._specs[7] = moved._specs[7][:1] + ((-1.2, 1.0, -1.0),) + moved._specs[7][2:]
    moved.finalize()
    tracer.update_transforms(moved)
    got = tracer.render(c, p)[1]
    fresh = render(tracer, moved, c, p)
    assert np.array_equal(bits(got), bits(fresh))
    assert not np.array_equal(bits(got), bits(render(tracer, scene, c, p)))


def test_replaced_light_mesh_equals_a_fresh_upload(tracer):
    w, h = 32, 24
    c = cam(w, h)
    p = lib.render_params(w, h, 4, 4, seed=10, shade_mode=NEE)
    scene = nee_ref.triangle_light_scene()
    tracer.upload_scene(scene)
    tracer.render(c, p)
    tris = scenes.load_mesh("cube").astype(np.float32).copy()
    tris[:, 0:9] *= np.float32(1.5)  # the vertices (normals and uvs stay)
    tracer.update_mesh(LIGHT_MESH, tris)
    got = tracer.render(c, p)[1]
    replaced = scenes.Scene()
    replaced._specs = list(scene._specs)
    kind, pos, rot, scl, _, bxdf = replaced._specs[LIGHT_MESH]
    replaced._specs[LIGHT_MESH] = (kind, pos, rot, scl, tris, bxdf)
    replaced.finalize()
    assert np.array_equal(bits(got), bits(render(tracer, replaced, c, p)))
    assert not np.array_equal(bits(got), bits(render(tracer, scene, c, p)))


# ---- isolation from the other modes, stats, refusals -----------------------------------------------------------------------

def test_nee_frames_leave_the_path_mode_and_gbuffer_alone(tracer):
    w, h = 40, 24
    c = cam(w, h)
    scene = scenes.cornell_wahoo_scene()
    p1 = lib.render_params(w, h, 4, 1, seed=3, shade_mode=PATH)
    p2 = lib.render_params(w, h, 4, 2, seed=4, shade_mode=PATH)
    pn = lib.render_params(w, h, 4, 3, seed=5, shade_mode=NEE)

    def sequence(t, with_nee):
        t.upload_scene(scene)
        out = []
        for step in ("p1", "p1", "gb", "p2", "p1", "gbn"):  # the second p1 finds the camera at rest: stored hits reused
            if with_nee:
                t.render(c, pn)
            if step == "gb":
                out.append(t.gbuffer(c, p1))
            elif step == "gbn":
                out.append(t.gbuffer(c, pn))
            else:
                out.append({"rad": t.render(c, p1 if step == "p1" else p2)[1]})
        return out

    with lib.Tracer(0) as fresh:
        a = sequence(fresh, False)
    b = sequence(tracer, True)
    for x, y in zip(a, b):
        for k in x:
            assert np.array_equal(x[k].view(np.uint8), y[k].view(np.uint8)), k


def test_stats_count_extension_and_shadow_rays(tracer):
    w, h = 32, 24
    c = cam(w, h)
    tracer.upload_scene(scenes.cornell_wahoo_scene())
    tracer.render(c, lib.render_params(w, h, 4, 4, seed=1, shade_mode=PATH, trace_mode=T.TRACE_BRUTE_FORCE))
    path_rays = tracer.stats().rays_traced
    tracer.render(c, lib.render_params(w, h, 4, 4, seed=1, shade_mode=NEE, trace_mode=T.TRACE_BRUTE_FORCE))
    st = tracer.stats()
    assert st.rays_traced > path_rays  # the same extension rays plus the shadow rays
    assert st.kernel_launches == 1 and st.kernel_ms > 0.0 and st.rays_answered == 0


def test_multi_device_entry_points_refuse_nee():
    with lib.MultiTracer([0]) as m:
        m.upload_scene(scenes.cornell_wahoo_scene())
        with pytest.raises(lib.FireflyError) as e:
            m.render(cam(16, 16), lib.render_params(16, 16, 2, 1, shade_mode=NEE))
        assert e.value.status == T.FF_ERR_UNSUPPORTED


# ---- the point of it: less variance --------------------------------------------------------------------------------------

def test_variance_on_c2_is_at_most_half(tracer):
    w, h = 160, 90
    c = cam(w, h)
    tracer.upload_scene(scenes.cornell_wahoo_scene())
    ref = tracer.render(c, lib.render_params(w, h, 8, 4096, seed=99, shade_mode=PATH))[1].astype(np.float64)
    mse = {}
    for mode in (PATH, NEE):
        img = tracer.render(c, lib.render_params(w, h, 8, 16, seed=7, shade_mode=mode))[1].astype(np.float64)
        mse[mode] = float(np.mean((img - ref) ** 2))
    assert mse[NEE] <= 0.5 * mse[PATH], mse
