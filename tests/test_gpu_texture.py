"""Albedo textures on the GPU: an all-ones texture changes no bit, the G-buffer's albedo plane against the host twins of the lookup
(exact for planes and meshes, within the reference's own sensitivity on spheres, the nearest texel or a neighbour under NEAREST),
direct lighting against the float64 reference, the furnace, PATH and NEE agreeing in expectation, determinism across trace modes,
launches, tiles, strips and progressive frames, exact scaling, updates of the scene, the refusals, and the denoiser's demodulation."""
import numpy as np
import pytest

from gpupathtracer_amd import lib, scenes
from gpupathtracer_amd import types as T
import nee_ref
import texture_ref

pytestmark = pytest.mark.gpu

NEE, PATH = T.SHADE_DIFFUSE_PATH_NEE, T.SHADE_DIFFUSE_PATH
INSIDE = dict(position=(0.0, 0.0, 2.4), yaw=-90.0, pitch=0.0)
OPEN = dict(position=(0.0, -1.2, 3.0), yaw=-90.0, pitch=0.0)
F = np.float32


def cam(w, h, pose=OPEN):
    return scenes.posed_camera(w, h, **pose)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def diffuse_geometries(scene):
    return [i for i in range(len(scene)) if scene.geometries[i].m_bxdf.contents.m_type == T.BXDF_DIFFUSE]


def albedo_of(scene, gi):
    a = scene.geometries[gi].m_bxdf.contents.m_albedo
    return np.array([a.x, a.y, a.z], F)


@pytest.fixture
def tex(tracer):
    """The session's tracer with a record of the textures a test creates: they are destroyed (and so unbound) afterwards."""
    made = []

    class Handle:
        t = tracer

        @staticmethod
        def create(rgb, flags=0):
            made.append(tracer.create_texture(rgb, flags))
            return made[-1]

    yield Handle
    for tid in made:
        try:
            tracer.destroy_texture(tid)
        except lib.FireflyError:
            pass  # (the test destroyed it itself)
    tracer.clear_environment()


def expected_albedo(scene, gb, bound, meshes):
    """m_albedo * ff_texture_sample(ff_surface_uv(position) * scale + offset) in float32 for every hit pixel of a bound geometry:
    bound = {geometry: (texels, flags, scale, offset)}, meshes = {geometry: float32 [n, 24] triangles}.  Returns (expected, mask)."""
    ids, pos = gb["ids"], gb["position"]
    out = np.zeros_like(gb["albedo"])
    mask = np.zeros(ids.shape[:2], bool)
    for gi, (texels, flags, scale, offset) in bound.items():
        m = ids[..., 0] == gi
        if not m.any():
            continue
        uv = lib.surface_uv(scene, gi, pos[m], ids[..., 1][m] if gi in meshes else None)
        c = (uv * np.asarray(scale, F) + np.asarray(offset, F)).astype(F)
        out[m] = albedo_of(scene, gi) * lib.texture_sample(texels, c, flags)
        mask |= m
    return out, mask


# ---- 1. an all-ones texture changes nothing -----------------------------------------------------------------------------------

@pytest.mark.parametrize("trace", [T.TRACE_BVH, T.TRACE_BRUTE_FORCE])
@pytest.mark.parametrize("spp", [1, 5, 130])
@pytest.mark.parametrize("jitter", [False, True])
def test_all_ones_texture_leaves_frames_bit_identical(tex, trace, spp, jitter):
    tracer = tex.t
    w, h = 24, 16
    c = cam(w, h, INSIDE)
    scene = scenes.cornell_wahoo_scene()
    ones = tex.create(np.ones((5, 7, 3), F))
    tracer.set_pixel_jitter(*(lib.jitter_sequence(3) if jitter else (0.0, 0.0)))
    try:
        for mode in (PATH, NEE):
            p = lib.render_params(w, h, 4, spp, seed=13, trace_mode=trace, shade_mode=mode)
            tracer.upload_scene(scene)
            a = tracer.render(c, p)
            ga = tracer.gbuffer(c, p)
            for gi in diffuse_geometries(scene):
                tracer.set_albedo_texture(gi, ones, scale=(3.0, 0.7), offset=(0.2, -0.4))
            b = tracer.render(c, p)
            assert tracer.kernel_name().startswith("nee_path_kernel") and tracer.kernel_name().endswith(", 1>")
            gb = tracer.gbuffer(c, p)
            assert np.array_equal(bits(a[1]), bits(b[1])), mode
            assert np.array_equal(a[0], b[0])
            assert a[1].max() > 0.0
            for k in ga:
                assert np.array_equal(ga[k].view(np.uint8), gb[k].view(np.uint8)), k
    finally:
        tracer.set_pixel_jitter(0.0, 0.0)


# ---- 2-4. the G-buffer's albedo plane -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("flags", [T.TEX_REPEAT, T.TEX_CLAMP])
@pytest.mark.parametrize("stored", [False, True])
def test_gbuffer_albedo_is_exact_on_planes_and_meshes(tex, flags, stored):
    tracer = tex.t
    wahoo = scenes.load_mesh("wahoo")
    scene = scenes.open_floor_scene(area_light=True, wahoo=wahoo)
    w, h = 96, 64
    c = cam(w, h)
    p = lib.render_params(w, h, 2, 2, seed=1, shade_mode=PATH)
    tracer.upload_scene(scene)
    if stored:
        tracer.render(c, p)  # (an untextured frame of two samples leaves its primary hits in the state: ff_gbuffer's other route)
    grad, check = scenes.gradient_texture(37, 23), scenes.checker_texture(16, 16, 4)
    bound = {0: (grad, flags, (1.0, 1.0), (0.0, 0.0)), 1: (check, flags, (6.0, 5.0), (0.13, 0.71))}
    for gi, (texels, fl, scale, offset) in bound.items():
        tracer.set_albedo_texture(gi, tex.create(texels, fl), scale, offset)
    gb = tracer.gbuffer(c, p)
    want, mask = expected_albedo(scene, gb, bound, {0: wahoo})
    assert (gb["ids"][..., 0] == 0).sum() > 200 and (gb["ids"][..., 0] == 1).sum() > 200
    assert np.array_equal(bits(gb["albedo"][mask]), bits(want[mask])), np.argwhere(np.any(gb["albedo"] != want, -1) & mask)[:5]
    assert len(np.unique(gb["albedo"][mask], axis=0)) > 100
    lamp = gb["ids"][..., 0] == 2
    assert np.all(gb["albedo"][lamp] == F(4.0) * np.array([1.0, 0.9, 0.8], F))  # (the emitter's plane is left alone)


def test_gbuffer_albedo_on_spheres_is_within_the_references_envelope(tex):
    tracer = tex.t
    s = scenes.Scene()
    s.add_sphere(1.0, (0.2, 0.1, 0.0), (10, 20, 30), (1.0, 1.3, 0.8), scenes.make_bxdf(T.BXDF_DIFFUSE, albedo=(1, 1, 1)))
    scene = s.finalize()
    w, h = 96, 64
    c = cam(w, h, dict(position=(0.0, 0.0, 3.0), yaw=-90.0, pitch=0.0))
    tracer.upload_scene(scene)
    grad = scenes.gradient_texture(64, 32)
    tracer.set_albedo_texture(0, tex.create(grad), (1.0, 1.0), (0.0, 0.0))
    gb = tracer.gbuffer(c, lib.render_params(w, h, 1, 1))
    m = gb["ids"][..., 0] == 0
    assert m.sum() > 500
    pos = gb["position"][m]
    # the host's atan2f / acosf may differ from the device's by an ulp: the reference at the position and at the position moved by
    # +-4 ulp of its largest component along each axis spans what such a difference can do
    step = (4.0 * np.spacing(np.abs(pos).max(1))).astype(F)
    vals = [lib.texture_sample(grad, lib.surface_uv(scene, 0, pos))]
    for axis in range(3):
        for sign in (-1.0, 1.0):
            q = pos.copy()
            q[:, axis] += F(sign) * step
            vals.append(lib.texture_sample(grad, lib.surface_uv(scene, 0, q)))
    vals = np.stack(vals).astype(np.float64)
    got = gb["albedo"][m].astype(np.float64)
    lo, hi = vals.min(0) - 1e-6, vals.max(0) + 1e-6
    assert np.all((got >= lo) & (got <= hi)), np.abs(got - vals[0]).max()
    assert got.std(0).min() > 0.01


@pytest.mark.parametrize("trace", [T.TRACE_BVH, T.TRACE_BRUTE_FORCE])
def test_nearest_shows_the_nearest_texel(tex, trace):
    tracer = tex.t
    wahoo = scenes.load_mesh("wahoo")
    scene = scenes.open_floor_scene(area_light=False, wahoo=wahoo)
    w, h = 96, 64
    c = cam(w, h)
    tracer.upload_scene(scene)
    rgb = np.random.default_rng(5).random((24, 40, 3)).astype(F)
    th, tw = rgb.shape[:2]
    tid = tex.create(rgb, T.TEX_NEAREST)
    scale, offset = {0: (1.0, 1.0), 1: (9.0, 7.0)}, {0: (0.0, 0.0), 1: (0.3, 0.6)}
    for gi in (0, 1):
        tracer.set_albedo_texture(gi, tid, scale[gi], offset[gi])
    gb = tracer.gbuffer(c, lib.render_params(w, h, 1, 1, trace_mode=trace))
    ids = gb["ids"]
    for gi in (0, 1):
        m = ids[..., 0] == gi
        assert m.sum() > 200
        uv = texture_ref.surface_uv64(scene, gi, gb["position"][m], wahoo, ids[..., 1][m])
        x, y = texture_ref.nearest_texel64(uv, tw, th, scale[gi], offset[gi])
        g = gb["albedo"][m]
        alb = albedo_of(scene, gi)
        exact = np.all(g == alb * rgb[y, x], -1)
        assert exact.mean() >= 0.95, f"{exact.mean():.4f} of geometry {gi}'s pixels show their texel"
        for i in np.nonzero(~exact)[0]:
            near = [alb * rgb[(y[i] + dy) % th, (x[i] + dx) % tw] for dy in (-1, 0, 1) for dx in (-1, 0, 1)]
            assert any(np.array_equal(g[i], n) for n in near), (gi, i, g[i])
    # the integrator multiplies the same texel in: one segment from a textured surface onto a white sky
    tracer.set_environment(np.ones((4, 8, 3), F))
    rad = tracer.render(c, lib.render_params(w, h, 2, 1, seed=3, trace_mode=trace, shade_mode=PATH))[1]
    floor = ids[..., 0] == 1
    lit = floor & np.any(rad > 0, -1)  # (paths that left the scene after the floor)
    assert lit.sum() > 100
    assert np.array_equal(bits(rad[lit]), bits(gb["albedo"][lit]))


# ---- 5. direct lighting against the float64 reference -----------------------------------------------------------------------------

@pytest.mark.parametrize("spp", [1, 2, 4])
def test_direct_lighting_matches_the_reference(tex, spp):
    tracer = tex.t
    scene = scenes.open_floor_scene(area_light=True)
    w, h = 96, 64
    c = cam(w, h)
    tracer.upload_scene(scene)
    tracer.set_albedo_texture(1, tex.create(scenes.gradient_texture(64, 64)), (12.0, 12.0), (0.0, 0.0))
    params = lib.render_params(w, h, bounces=2, spp=spp, seed=2024, shade_mode=NEE)
    got = tracer.render(c, params)[1].astype(np.float64)
    assert tracer.kernel_name().endswith(", 0, 1>")
    ref, hit, excused = nee_ref.direct_lighting(tracer, scene, c, params)  # (beta comes from the G-buffer's textured albedo)
    ok = np.all(np.abs(got - ref) <= 1e-4 * np.abs(ref) + 1e-6, -1)
    frac = ok[hit].mean()
    print(f"spp {spp}: {frac:.5f} of {hit.sum()} hit pixels within tolerance, {excused[hit].mean():.5f} excused, {(hit & ~ok & ~excused).sum()} unexcused")
    assert frac >= 0.995, f"{frac:.4f} of hit pixels within tolerance"
    bad = hit & ~ok & ~excused
    assert not bad.any(), f"{bad.sum()} pixels off the reference that no ray decision excuses: {np.argwhere(bad)[:5]}"
    assert excused[hit].mean() <= 0.05
    assert (ref[hit] > 0).any()


# ---- 6. furnace ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", [PATH, NEE])
def test_furnace(tex, mode):
    tracer = tex.t
    s = scenes.Scene()
    s.add_sphere(1.0, (0.0, 0.0, 0.0), (0, 0, 0), (1, 1, 1), scenes.make_bxdf(T.BXDF_DIFFUSE, albedo=(1, 1, 1)))
    scene = s.finalize()
    w, h = 64, 48
    c = cam(w, h, dict(position=(0.0, 0.0, 3.0), yaw=-90.0, pitch=0.0))
    tracer.upload_scene(scene)
    tracer.set_albedo_texture(0, tex.create(np.full((8, 8, 3), 0.5, F)))
    tracer.set_environment(np.full((16, 32, 3), 0.5, F))
    miss = tracer.gbuffer(c, lib.render_params(w, h, 1, 1))["ids"][..., 0] < 0
    got = tracer.render(c, lib.render_params(w, h, 4, 64, seed=17, shade_mode=mode))[1].astype(np.float64)
    assert tracer.kernel_name().endswith(", 1, 1>")
    assert np.all(got[miss] == 0.5)
    mean = got[~miss].mean()
    assert abs(mean - 0.25) <= 0.01 * 0.25, mean


# ---- 7. PATH and NEE agree in expectation ---------------------------------------------------------------------------------------------

def textured_box(tex):
    tracer = tex.t
    scene = scenes.cornell_wahoo_scene()
    tracer.upload_scene(scene)
    grad = tex.create(scenes.gradient_texture(48, 48))
    check = tex.create(scenes.checker_texture(32, 32, 4), T.TEX_NEAREST)
    for n, gi in enumerate(diffuse_geometries(scene)):
        tracer.set_albedo_texture(gi, grad if n % 2 == 0 else check, (2.0, 2.0), (0.1 * n, 0.0))
    return scene


def test_same_expectation_path_and_nee(tex):
    tracer = tex.t
    w, h, seeds = 48, 32, 16
    c = cam(w, h, dict(position=(0.0, 0.0, 6.0), yaw=-90.0, pitch=0.0))
    textured_box(tex)
    imgs = {}
    for mode in (PATH, NEE):
        imgs[mode] = np.stack([tracer.render(c, lib.render_params(w, h, 6, 32, seed=1000 + s, shade_mode=mode))[1] for s in range(seeds)]).astype(np.float64)
    assert imgs[PATH].mean() > 0.0

    def blocks(x):
        return x.reshape(seeds, h // 8, 8, w // 8, 8, 3).mean(axis=(2, 4))

    a, b = blocks(imgs[PATH]), blocks(imgs[NEE])
    se = np.sqrt(a.var(0, ddof=1) / seeds + b.var(0, ddof=1) / seeds) + 1e-7
    z = np.abs(a.mean(0) - b.mean(0)) / se
    assert z.max() < 5.0, f"block mean off by {z.max():.2f} standard errors"
    ia, ib = imgs[PATH].mean(axis=(1, 2, 3)), imgs[NEE].mean(axis=(1, 2, 3))
    zi = abs(ia.mean() - ib.mean()) / np.sqrt(ia.var(ddof=1) / seeds + ib.var(ddof=1) / seeds)
    assert zi < 4.0, f"image mean off by {zi:.2f} standard errors"


# ---- 8. determinism and partitioning ----------------------------------------------------------------------------------------------

def test_repeatable_and_bvh_equals_brute_force(tex):
    tracer = tex.t
    textured_box(tex)
    w, h = 40, 30
    c = cam(w, h, INSIDE)
    for mode in (PATH, NEE):
        p = lib.render_params(w, h, 5, 9, seed=5, shade_mode=mode)
        a = tracer.render(c, p)[1]
        assert np.array_equal(bits(a), bits(tracer.render(c, p)[1]))
        p.trace_mode = T.TRACE_BRUTE_FORCE
        assert np.array_equal(bits(a), bits(tracer.render(c, p)[1])), mode


def test_independent_of_spp_per_launch(tex):
    tracer = tex.t
    textured_box(tex)
    w, h = 32, 24
    c = cam(w, h, INSIDE)
    ref = tracer.render(c, lib.render_params(w, h, 4, 200, seed=8, shade_mode=NEE))[1]
    for spl in (1, 64, 128):
        got = tracer.render(c, lib.render_params(w, h, 4, 200, seed=8, shade_mode=NEE, spp_per_launch=spl))[1]
        assert np.array_equal(bits(ref), bits(got)), spl


def test_tiles_strips_and_progressive(tex):
    tracer = tex.t
    textured_box(tex)
    w, h = 44, 30
    c = cam(w, h, INSIDE)
    for mode in (PATH, NEE):
        p = lib.render_params(w, h, 4, 3, seed=21, shade_mode=mode)
        full = tracer.render(c, p)[1]
        for (x0, y0, tw, th) in ((0, 0, 16, 8), (13, 7, 20, 17), (40, 25, 4, 5)):
            tile = tracer.render_tile(c, p, x0, y0, tw, th)[1]
            assert np.array_equal(bits(tile), bits(full[y0:y0 + th, x0:x0 + tw])), (x0, y0)
        strip_rows, parts = 4, 3
        for part in range(parts):
            _, srad = tracer.render_strips(c, p, strip_rows, part, parts)
            rows = [y for y in range(h) if (y // strip_rows) % parts == part]
            assert np.array_equal(bits(srad), bits(full[rows])), part
        acc = None
        for i in range(3):
            frame = tracer.render(c, lib.render_params(w, h, 4, 2, seed=300 + i, shade_mode=mode))[1]
            _, mean = tracer.render_progressive(c, lib.render_params(w, h, 4, 2, seed=300, shade_mode=mode), i)
            acc = frame.copy() if i == 0 else acc + frame
            assert np.array_equal(bits(mean), bits(acc * np.float32(1.0 / (i + 1))))


# ---- 9. exact scaling -----------------------------------------------------------------------------------------------------------------

def test_doubling_the_texels_doubles_the_albedo_plane(tex):
    tracer = tex.t
    scene = scenes.open_floor_scene(area_light=False)
    w, h = 64, 48
    c = cam(w, h)
    p = lib.render_params(w, h, 1, 1)
    tracer.upload_scene(scene)
    rgb = (0.5 * np.random.default_rng(8).random((19, 33, 3))).astype(F)
    planes = []
    for texels in (rgb, rgb * F(2.0)):
        tid = tex.create(texels)
        for gi in (0, 1):
            tracer.set_albedo_texture(gi, tid, (3.0, 3.0), (0.25, 0.5))
        planes.append(tracer.gbuffer(c, p)["albedo"])
    assert planes[0].max() > 0.0
    assert np.array_equal(bits(planes[1]), bits(planes[0] * F(2.0)))


# ---- 10. updates ------------------------------------------------------------------------------------------------------------------------

def test_update_transforms_keeps_the_binding(tex):
    tracer = tex.t
    wahoo = scenes.load_mesh("wahoo")
    scene = scenes.open_floor_scene(area_light=True, wahoo=wahoo)
    w, h = 64, 48
    c = cam(w, h)
    p = lib.render_params(w, h, 1, 1)
    tracer.upload_scene(scene)
    grad = scenes.gradient_texture(37, 23)
    bound = {0: (grad, 0, (1.0, 1.0), (0.0, 0.0)), 1: (grad, 0, (5.0, 5.0), (0.0, 0.5))}
    tid = tex.create(grad)
    for gi, (_, _, scale, offset) in bound.items():
        tracer.set_albedo_texture(gi, tid, scale, offset)
    moved = scenes.Scene()
    moved.add_mesh(wahoo, (0.4, -2.4, 0.2), (0, 35, 0), (0.3, 0.3, 0.3), scenes.make_bxdf(T.BXDF_DIFFUSE, albedo=(0.8, 0.3, 0.2)))
    moved.add_plane((0, -2.5, 0), (90, 0, 0), (30, 30, 30), scenes.make_bxdf(T.BXDF_DIFFUSE, albedo=(0.6, 0.6, 0.6)))
    moved.add_plane((1.0, 0.5, 0.5), (90, 0, 0), (1.5, 1.5, 1.5), scenes.make_bxdf(T.BXDF_EMITTER, emissive=(1.0, 0.9, 0.8), intensity=4.0))
    moved.finalize()
    tracer.update_transforms(moved)
    gb = tracer.gbuffer(c, p)
    want, mask = expected_albedo(moved, gb, bound, {0: wahoo})
    assert mask.sum() > 500
    assert np.array_equal(bits(gb["albedo"][mask]), bits(want[mask]))


@pytest.mark.parametrize("builder,mode", [(T.BUILD_HOST_SAH, T.UPDATE_REFIT), (T.BUILD_GPU_LBVH, T.UPDATE_REFIT), (T.BUILD_GPU_LBVH, T.UPDATE_REBUILD),
                                          (T.BUILD_GPU_PLOC, T.UPDATE_REFIT), (T.BUILD_GPU_PLOC, T.UPDATE_REBUILD)])
def test_update_mesh_samples_the_new_uvs(tex, builder, mode):
    tracer = tex.t
    wahoo = scenes.load_mesh("wahoo")
    scene = scenes.open_floor_scene(area_light=False, wahoo=wahoo)
    w, h = 64, 48
    c = cam(w, h)
    p = lib.render_params(w, h, 1, 1)
    grad = scenes.gradient_texture(37, 23)
    bound = {0: (grad, 0, (1.0, 1.0), (0.0, 0.0))}
    tracer.set_builder(builder)
    try:
        tracer.upload_scene(scene)
        tracer.set_albedo_texture(0, tex.create(grad))
        gb = tracer.gbuffer(c, p)
        want, mask = expected_albedo(scene, gb, bound, {0: wahoo})
        assert mask.sum() > 200 and np.array_equal(bits(gb["albedo"][mask]), bits(want[mask]))  # (every builder's UV side array)
        swapped = wahoo.copy()
        swapped[:, [9, 11, 13]], swapped[:, [10, 12, 14]] = wahoo[:, [10, 12, 14]], wahoo[:, [9, 11, 13]]
        tracer.update_mesh(0, swapped, mode)
        after = scenes.open_floor_scene(area_light=False, wahoo=swapped)
        gb2 = tracer.gbuffer(c, p)
        want2, mask2 = expected_albedo(after, gb2, bound, {0: swapped})
        assert np.array_equal(mask, mask2)
        assert np.array_equal(bits(gb2["albedo"][mask2]), bits(want2[mask2]))
        assert not np.array_equal(gb2["albedo"][mask2], gb["albedo"][mask])
    finally:
        tracer.set_builder(T.BUILD_HOST_SAH)


def test_upload_drops_bindings_and_destroy_unbinds(tex):
    tracer = tex.t
    scene = scenes.open_floor_scene(area_light=True)
    w, h = 48, 32
    c = cam(w, h)
    p = lib.render_params(w, h, 3, 4, seed=6, shade_mode=NEE)
    tracer.upload_scene(scene)
    plain = tracer.render(c, p)[1]
    plain_gb = tracer.gbuffer(c, p)["albedo"]
    tid = tex.create(scenes.checker_texture(16, 16, 4))
    tracer.set_albedo_texture(1, tid, (10.0, 10.0))
    textured = tracer.render(c, p)[1]
    assert not np.array_equal(textured, plain)
    tracer.upload_scene(scene)  # (bindings belong to the scene; the texture stays)
    assert np.array_equal(bits(plain), bits(tracer.render(c, p)[1]))
    assert np.array_equal(bits(plain_gb), bits(tracer.gbuffer(c, p)["albedo"]))
    tracer.set_albedo_texture(1, tid, (10.0, 10.0))
    assert np.array_equal(bits(textured), bits(tracer.render(c, p)[1]))
    tracer.set_albedo_texture(1, None)
    assert np.array_equal(bits(plain), bits(tracer.render(c, p)[1]))
    assert not tracer.kernel_name().endswith(", 0, 1>")
    tracer.set_albedo_texture(1, tid, (10.0, 10.0))
    tracer.destroy_texture(tid)
    assert np.array_equal(bits(plain), bits(tracer.render(c, p)[1]))
    assert np.array_equal(bits(plain_gb), bits(tracer.gbuffer(c, p)["albedo"]))
    with pytest.raises(lib.FireflyError) as e:
        tracer.set_albedo_texture(1, tid)
    assert e.value.status == T.FF_ERR_INVALID_ARG


# ---- 11. refusals -------------------------------------------------------------------------------------------------------------------------

def test_argument_checks_and_refusals(tex):
    tracer = tex.t
    w, h = 16, 16
    c = cam(w, h, INSIDE)
    scene = scenes.cornell_glass_scene()
    tracer.upload_scene(scene)
    ok = np.full((2, 2, 3), 0.5, F)
    for bad in (-0.1, np.nan, np.inf):
        t = ok.copy()
        t[0, 1, 2] = bad
        with pytest.raises(lib.FireflyError) as e:
            tracer.create_texture(t)
        assert e.value.status == T.FF_ERR_INVALID_ARG
    for flags in (4, 7, 256):
        with pytest.raises(lib.FireflyError) as e:
            tracer.create_texture(ok, flags)
        assert e.value.status == T.FF_ERR_INVALID_ARG
    tid = tex.create(ok)
    kinds = {scene.geometries[i].m_bxdf.contents.m_type: i for i in range(len(scene))}
    assert T.BXDF_EMITTER in kinds and T.BXDF_GLASS in kinds
    for kind in (T.BXDF_EMITTER, T.BXDF_GLASS):
        with pytest.raises(lib.FireflyError) as e:
            tracer.set_albedo_texture(kinds[kind], tid)
        assert e.value.status == T.FF_ERR_UNSUPPORTED
    tracer.upload_scene(scenes.cornell_mirror_scene())
    ms = scenes.cornell_mirror_scene()
    mirror = [i for i in range(len(ms)) if ms.geometries[i].m_bxdf.contents.m_type == T.BXDF_MIRROR][0]
    with pytest.raises(lib.FireflyError) as e:
        tracer.set_albedo_texture(mirror, tid)
    assert e.value.status == T.FF_ERR_UNSUPPORTED
    for args in ((99, tid), (-1, tid), (0, 57), (0, -2)):
        with pytest.raises(lib.FireflyError) as e:
            tracer.set_albedo_texture(*args)
        assert e.value.status == T.FF_ERR_INVALID_ARG
    with pytest.raises(lib.FireflyError) as e:
        tracer.set_albedo_texture(diffuse_geometries(ms)[0], tid, (np.nan, 1.0))
    assert e.value.status == T.FF_ERR_INVALID_ARG
    with pytest.raises(lib.FireflyError) as e:
        tracer.destroy_texture(1234)
    assert e.value.status == T.FF_ERR_INVALID_ARG
    # SMOOTH refuses while a binding exists; NORMAL_DEBUG ignores it
    scene = scenes.cornell_wahoo_scene()
    tracer.upload_scene(scene)
    pd = lib.render_params(w, h, 1, 1, shade_mode=T.SHADE_NORMAL_DEBUG)
    ps = lib.render_params(w, h, 2, 1, shade_mode=T.SHADE_DIFFUSE_PATH_SMOOTH)
    dbg = tracer.render(c, pd)
    smooth = tracer.render(c, ps)[1]
    tracer.set_albedo_texture(diffuse_geometries(scene)[0], tid)
    with pytest.raises(lib.FireflyError) as e:
        tracer.render(c, ps)
    assert e.value.status == T.FF_ERR_UNSUPPORTED
    again = tracer.render(c, pd)
    assert np.array_equal(bits(dbg[1]), bits(again[1])) and np.array_equal(dbg[0], again[0])
    tracer.set_albedo_texture(diffuse_geometries(scene)[0], None)
    assert np.array_equal(bits(smooth), bits(tracer.render(c, ps)[1]))


def test_multi_device_entry_points_refuse(tex):
    w, h = 16, 16
    c = cam(w, h)
    ok = np.full((2, 2, 3), 0.5, F)
    with lib.MultiTracer([0]) as m:
        m.upload_scene(scenes.open_floor_scene(False))
        st = m._lib.ff_multi_state(m._handle, 0)
        tid = lib.C.c_int(-1)
        lib.check(m._lib.ff_texture_create(st, ok.ctypes.data, 2, 2, 0, lib.C.byref(tid)))
        m.render(c, lib.render_params(w, h, 2, 1, shade_mode=PATH))  # (a texture alone refuses nothing)
        lib.check(m._lib.ff_set_albedo_texture(st, 1, tid.value, 1.0, 1.0, 0.0, 0.0))
        for mode in (PATH, NEE):
            with pytest.raises(lib.FireflyError) as e:
                m.render(c, lib.render_params(w, h, 2, 1, shade_mode=mode))
            assert e.value.status == T.FF_ERR_UNSUPPORTED
        m.render(c, lib.render_params(w, h, 2, 1, shade_mode=T.SHADE_NORMAL_DEBUG))  # (the debug view renders)


def test_distributed_entry_point_refuses():
    """On a one-rank communicator (a tracer of its own, as tests/test_gpu_dist.py sets it up)."""
    if not lib.dist_available():
        pytest.fail("the RCCL library is not loadable: ff_render_distributed cannot be exercised")
    w, h = 16, 16
    c = cam(w, h)
    with lib.Tracer(0) as t:
        t.upload_scene(scenes.open_floor_scene(False))
        t.dist_init(0, 1, lib.dist_unique_id())
        try:
            p = lib.render_params(w, h, 2, 1, shade_mode=PATH)
            plain = t.render_distributed(c, p)[1]
            tid = t.create_texture(np.full((2, 2, 3), 0.5, F))
            assert np.array_equal(bits(plain), bits(t.render_distributed(c, p)[1]))  # (a texture alone refuses nothing)
            t.set_albedo_texture(1, tid)
            with pytest.raises(lib.FireflyError) as e:
                t.render_distributed(c, p)
            assert e.value.status == T.FF_ERR_UNSUPPORTED
            t.render_distributed(c, lib.render_params(w, h, 1, 1, shade_mode=T.SHADE_NORMAL_DEBUG))
            t.set_albedo_texture(1, None)
            assert np.array_equal(bits(plain), bits(t.render_distributed(c, p)[1]))
        finally:
            t.dist_shutdown()


# ---- 12. the denoiser's demodulation earns its keep -----------------------------------------------------------------------------------------

def test_demodulation_lowers_the_error_on_a_textured_floor(tex):
    tracer = tex.t
    scene = scenes.open_floor_scene(area_light=True)
    w, h = 160, 96
    c = cam(w, h)
    tracer.upload_scene(scene)
    tracer.set_albedo_texture(1, tex.create(scenes.checker_texture(64, 64, 8), T.TEX_NEAREST), (16.0, 16.0))
    noisy = tracer.render(c, lib.render_params(w, h, 4, 16, seed=1, shade_mode=NEE))[1]
    truth = tracer.render(c, lib.render_params(w, h, 4, 1024, seed=99, shade_mode=NEE))[1].astype(np.float64)
    gb = tracer.gbuffer(c, lib.render_params(w, h, 1, 1))
    mse = {}
    for name, flags in (("demodulated", T.DENOISE_SAME_GEOMETRY | T.DENOISE_DEMODULATE_ALBEDO), ("plain", T.DENOISE_SAME_GEOMETRY)):
        out = tracer.denoise(noisy, gb, lib.denoise_params(flags=flags))[1].astype(np.float64)
        mse[name] = float(np.mean((out - truth) ** 2))
    raw = float(np.mean((noisy.astype(np.float64) - truth) ** 2))
    print(f"MSE against 1024 spp: raw {raw:.5g}, à-trous without demodulation {mse['plain']:.5g}, with {mse['demodulated']:.5g}")
    assert mse["demodulated"] < mse["plain"], mse
