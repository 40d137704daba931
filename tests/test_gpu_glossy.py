"""Rough-specular (GGX) mirrors on the GPU (ff_set_roughness): frames without an applied binding stay bit for bit what they were,
direct lighting against the float64 reference (tests/glossy_ref.py), agreement in expectation between FF_SHADE_DIFFUSE_PATH and
FF_SHADE_DIFFUSE_PATH_NEE, the furnace bound, determinism across trace modes, launches, tiles, strips and progressive frames,
dynamic scenes, isolation from the other modes and ff_gbuffer, and the refusals."""
import ctypes as C

import numpy as np
import pytest

from gpupathtracer_amd import lib, scenes
from gpupathtracer_amd import types as T
import glossy_ref
import nee_ref

pytestmark = pytest.mark.gpu

NEE, PATH = T.SHADE_DIFFUSE_PATH_NEE, T.SHADE_DIFFUSE_PATH
INSIDE = dict(position=(0.0, 0.0, 2.4), yaw=-90.0, pitch=0.0)
OUTSIDE = dict(position=(0.0, 0.6, 4.0), yaw=-90.0, pitch=-8.0)
C2_FLOOR, TRI_FLOOR, TRI_BACK, TRI_CUBE = 3, 2, 1, 0  # geometry indices in scenes.cornell_wahoo_scene / nee_ref.triangle_light_scene


def cam(w, h, **pose):
    return scenes.posed_camera(w, h, **(pose or INSIDE))


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def mirrors(scene):
    return [i for i in range(len(scene)) if scene.geometries[i].m_bxdf.contents.m_type == T.BXDF_MIRROR]


def is_glossy_kernel(name):
    """nee_path_kernel<MODE, BIG, ENV, TEX, 1>: the instantiations with GLOSSY are the ones named by all five parameters."""
    return name.startswith("nee_path_kernel<") and name.count(",") == 4 and name.endswith(", 1>")


def one_texel_map(value=400.0, floor=0.0):
    env = np.full((8, 16, 3), floor, np.float32)
    env[2, 5] = (value, 0.9 * value, 0.7 * value)
    return env


@pytest.fixture
def gl(tracer):
    """The session's tracer, without an environment before and after."""
    tracer.clear_environment()
    yield tracer
    tracer.clear_environment()


def bound_upload(tracer, scene, roughness):
    tracer.upload_scene(scene)
    for g, r in roughness.items():
        tracer.set_roughness(g, r)


# ---- 1. nothing bound, nothing changes ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["C2", "mirror"])
@pytest.mark.parametrize("mode", [PATH, NEE])
@pytest.mark.parametrize("trace", [T.TRACE_BVH, T.TRACE_BRUTE_FORCE])
@pytest.mark.parametrize("spp", [1, 130])
def test_nothing_bound_nothing_changes(gl, name, mode, trace, spp):
    scene = scenes.cornell_wahoo_scene() if name == "C2" else scenes.cornell_mirror_scene()
    w, h = 24, 16
    c = cam(w, h)
    p = lib.render_params(w, h, 4, spp, seed=17, trace_mode=trace, shade_mode=mode)
    with lib.Tracer(0) as fresh:
        fresh.upload_scene(scene)
        want = fresh.render(c, p)
        want_kernel = fresh.kernel_name()
    gl.upload_scene(scene)
    targets = mirrors(scene)
    if targets:
        for g in targets:
            gl.set_roughness(g, 0.4)
        bound = gl.render(c, p)[1]
        assert is_glossy_kernel(gl.kernel_name()) and not np.array_equal(bits(bound), bits(want[1]))
        for g in targets:
            gl.set_roughness(g, 0.0)
    else:
        with pytest.raises(lib.FireflyError) as e:
            gl.set_roughness(C2_FLOOR, 0.4)
        assert e.value.status == T.FF_ERR_UNSUPPORTED
        gl.set_roughness(C2_FLOOR, 0.0)
    got = gl.render(c, p)
    assert gl.kernel_name() == want_kernel
    assert np.array_equal(bits(got[1]), bits(want[1])) and np.array_equal(got[0], want[0])
    # alpha = 0.02^2 < 1e-3: the binding is applied, and shades as the perfect mirror
    for g in targets:
        gl.set_roughness(g, 0.02)
    got = gl.render(c, p)
    assert np.array_equal(bits(got[1]), bits(want[1])) and np.array_equal(got[0], want[0])
    if targets:
        assert is_glossy_kernel(gl.kernel_name()) and not is_glossy_kernel(want_kernel)


# ---- 2. direct lighting against the float64 reference ---------------------------------------------------------------------------

def check_direct(got, ref, hit, excused):
    """test_gpu_nee.py's test_direct_lighting_matches_the_reference rule."""
    ok = np.all(np.abs(got - ref) <= 1e-4 * np.abs(ref) + 1e-6, -1)
    frac = ok[hit].mean()
    print(f"within tolerance {frac:.5f}, excused {excused[hit].mean():.5f}, off and unexcused {(hit & ~ok & ~excused).sum()}")
    assert frac >= 0.995, f"{frac:.4f} of hit pixels within tolerance"
    bad = hit & ~ok & ~excused
    assert not bad.any(), f"{bad.sum()} pixels off the reference that no ray decision excuses: {np.argwhere(bad)[:5]}"
    assert excused[hit].mean() <= 0.05
    assert (ref[hit] > 0).any()


@pytest.mark.parametrize("name,geom", [("C2", C2_FLOOR), ("triangle_lights", TRI_BACK)])
@pytest.mark.parametrize("rough", [0.3, 0.6])
@pytest.mark.parametrize("spp", [1, 4])
def test_direct_lighting_matches_the_reference(gl, name, geom, rough, spp):
    base = scenes.cornell_wahoo_scene() if name == "C2" else nee_ref.triangle_light_scene()
    scene = glossy_ref.with_mirror(base, geom)
    w, h = 96, 64
    c = cam(w, h)
    params = lib.render_params(w, h, bounces=2, spp=spp, seed=2024, shade_mode=NEE)
    bound_upload(gl, scene, {geom: rough})
    got = gl.render(c, params)[1].astype(np.float64)
    ref, hit, excused = glossy_ref.direct_lighting(gl, scene, c, params, {geom: rough})
    glossy_px = gl.gbuffer(c, params)["ids"][..., 0] == geom
    assert glossy_px.sum() > 200 and (ref[glossy_px] > 0).any()
    check_direct(got, ref, hit, excused)


@pytest.mark.parametrize("spp", [1, 4])
def test_direct_lighting_under_an_environment(gl, spp):
    scene = glossy_ref.sphere_on_floor_scene()
    env = one_texel_map()
    w, h = 96, 64
    c = cam(w, h, **OUTSIDE)
    params = lib.render_params(w, h, bounces=2, spp=spp, seed=77, shade_mode=NEE)
    bound_upload(gl, scene, {0: 0.3})
    gl.set_environment(env, 1.0, 20.0)
    got = gl.render(c, params)[1].astype(np.float64)
    ref, hit, excused = glossy_ref.direct_lighting(gl, scene, c, params, {0: 0.3}, env=(env, 1.0, 20.0))
    glossy_px = gl.gbuffer(c, params)["ids"][..., 0] == 0
    assert glossy_px.sum() > 300 and (ref[glossy_px] > 0).any()
    check_direct(got, ref, hit, excused)


# ---- 3. same expectation in both modes ------------------------------------------------------------------------------------------

def rough_c2():
    return glossy_ref.with_mirror(scenes.cornell_wahoo_scene(), C2_FLOOR), {C2_FLOOR: 0.3}, INSIDE, None


def rough_mirror_scene():
    s = scenes.cornell_mirror_scene()
    return s, {g: 0.15 for g in mirrors(s)}, INSIDE, None


def rough_sphere_env():
    return glossy_ref.sphere_on_floor_scene(), {0: 0.3}, OUTSIDE, one_texel_map(60.0, 0.4)


@pytest.mark.parametrize("make", [rough_c2, rough_mirror_scene, rough_sphere_env])
def test_same_expectation_as_the_path_mode(gl, make):
    """test_gpu_nee.py's z-test, unchanged."""
    scene, roughness, pose, env = make()
    w, h, seeds = 48, 32, 16
    c = cam(w, h, **pose)
    bound_upload(gl, scene, roughness)
    if env is not None:
        gl.set_environment(env)
    imgs = {}
    for mode in (PATH, NEE):
        imgs[mode] = np.stack([gl.render(c, lib.render_params(w, h, 8, 32, seed=1000 + s, shade_mode=mode))[1] for s in range(seeds)]).astype(np.float64)
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


# ---- 4. furnace -------------------------------------------------------------------------------------------------------------------

def test_furnace_bound(gl):
    scene = glossy_ref.lone_sphere_scene((1.0, 1.0, 1.0))
    w, h = 32, 32
    c = cam(w, h, position=(0.0, 0.0, 3.0), yaw=-90.0, pitch=0.0)
    p = lib.render_params(w, h, 8, 64, seed=5, shade_mode=PATH)
    bound_upload(gl, scene, {0: 0.5})
    gl.set_environment(np.ones((2, 4, 3), np.float32))
    rad = gl.render(c, p)[1]
    on = gl.gbuffer(c, p)["ids"][..., 0] == 0
    assert on.sum() > 100 and (~on).sum() > 100
    assert rad.max() <= 1.0 + 1e-5
    assert (rad[on] > 0.0).all()
    assert (rad[~on] == 1.0).all()
    assert rad[on].mean() < 0.999  # (single scattering loses energy: no compensation is offered)


# ---- 5. determinism -----------------------------------------------------------------------------------------------------------------

@pytest.fixture
def rough_tri(gl):
    scene = glossy_ref.with_mirror(nee_ref.triangle_light_scene(), TRI_FLOOR)
    bound_upload(gl, scene, {TRI_FLOOR: 0.3})
    return gl


@pytest.mark.parametrize("mode", [PATH, NEE])
def test_repeatable_and_bvh_equals_brute_force(rough_tri, mode):
    w, h = 40, 30
    c = cam(w, h)
    p = lib.render_params(w, h, 5, 9, seed=5, shade_mode=mode)
    a = rough_tri.render(c, p)[1]
    assert a.max() > 0.0 and is_glossy_kernel(rough_tri.kernel_name())
    assert np.array_equal(bits(a), bits(rough_tri.render(c, p)[1]))
    p.trace_mode = T.TRACE_BRUTE_FORCE
    assert np.array_equal(bits(a), bits(rough_tri.render(c, p)[1]))


def test_independent_of_spp_per_launch(rough_tri):
    w, h = 40, 30
    c = cam(w, h)
    ref = rough_tri.render(c, lib.render_params(w, h, 4, 200, seed=8, shade_mode=NEE))[1]
    for spl in (1, 64, 128):
        got = rough_tri.render(c, lib.render_params(w, h, 4, 200, seed=8, shade_mode=NEE, spp_per_launch=spl))[1]
        assert np.array_equal(bits(ref), bits(got)), spl


def test_tiles_and_strips_match_the_full_frame(rough_tri):
    w, h = 40, 30
    c = cam(w, h)
    p = lib.render_params(w, h, 4, 3, seed=21, shade_mode=NEE)
    full = rough_tri.render(c, p)[1]
    for (x0, y0, tw, th) in ((0, 0, 16, 8), (13, 7, 20, 17), (36, 25, 4, 5)):
        tile = rough_tri.render_tile(c, p, x0, y0, tw, th)[1]
        assert np.array_equal(bits(tile), bits(full[y0:y0 + th, x0:x0 + tw])), (x0, y0)
    strip_rows, parts = 4, 3
    for part in range(parts):
        _, srad = rough_tri.render_strips(c, p, strip_rows, part, parts)
        rows = [y for y in range(h) if (y // strip_rows) % parts == part]
        assert np.array_equal(bits(srad), bits(full[rows])), part


def test_progressive_is_the_mean_of_its_frames(rough_tri):
    w, h = 40, 30
    c = cam(w, h)
    frames, acc = [], None
    for i in range(4):
        frames.append(rough_tri.render(c, lib.render_params(w, h, 4, 2, seed=300 + i, shade_mode=NEE))[1])
        _, mean = rough_tri.render_progressive(c, lib.render_params(w, h, 4, 2, seed=300, shade_mode=NEE), i)
        acc = frames[0].copy() if i == 0 else acc + frames[i]
        assert np.array_equal(bits(mean), bits(acc * np.float32(1.0 / (i + 1))))


def test_emission_scales_exactly(gl):
    w, h = 40, 30
    c = cam(w, h)
    p = lib.render_params(w, h, 6, 4, seed=4, shade_mode=NEE)
    out = []
    for k in (1.0, 2.0):
        bound_upload(gl, glossy_ref.with_mirror(nee_ref.triangle_light_scene(k), TRI_FLOOR), {TRI_FLOOR: 0.3})
        out.append(gl.render(c, p)[1])
    assert out[0].max() > 0.0
    assert np.array_equal(bits(out[1]), bits(out[0] * np.float32(2.0)))


# ---- 6. dynamic scenes ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("builder", [T.BUILD_HOST_SAH, T.BUILD_GPU_LBVH, T.BUILD_GPU_PLOC])
def test_bindings_survive_the_update_calls(gl, builder):
    w, h = 40, 30
    c = cam(w, h)
    p = lib.render_params(w, h, 4, 4, seed=9, shade_mode=NEE)
    scene = glossy_ref.with_mirror(nee_ref.triangle_light_scene(), TRI_CUBE)
    roughness = {TRI_CUBE: 0.35}
    gl.set_builder(builder)
    try:
        bound_upload(gl, scene, roughness)
        first = gl.render(c, p)[1]
        # new transforms
        moved = scenes.Scene()
        moved._specs = list(scene._specs)
        kind, pos, rot, scl, tris, bxdf = moved._specs[TRI_CUBE]
        moved._specs[TRI_CUBE] = (kind, (0.1, -1.8, -0.2), (10, 60, 0), (1.2, 1.0, 1.1), tris, bxdf)
        moved.finalize()
        gl.update_transforms(moved)
        got = gl.render(c, p)[1]
        assert is_glossy_kernel(gl.kernel_name()) and not np.array_equal(bits(got), bits(first))
        bound_upload(gl, moved, roughness)
        assert np.array_equal(bits(got), bits(gl.render(c, p)[1]))
        # new vertices
        tris2 = scenes.load_mesh("cube").astype(np.float32).copy()
        tris2[:, 0:9] *= np.float32(1.3)
        gl.update_mesh(TRI_CUBE, tris2)
        got = gl.render(c, p)[1]
        replaced = scenes.Scene()
        replaced._specs = list(moved._specs)
        replaced._specs[TRI_CUBE] = replaced._specs[TRI_CUBE][:4] + (tris2, replaced._specs[TRI_CUBE][5])
        replaced.finalize()
        bound_upload(gl, replaced, roughness)
        assert np.array_equal(bits(got), bits(gl.render(c, p)[1]))
        # a geometry the update makes diffuse keeps its binding, which is not applied - and is again once it is a mirror again
        plain = scenes.Scene()
        plain._specs = list(replaced._specs)
        plain._specs[TRI_CUBE] = plain._specs[TRI_CUBE][:5] + (scenes.make_bxdf(T.BXDF_DIFFUSE, albedo=(0.8, 0.8, 0.8)),)
        plain.finalize()
        gl.update_transforms(plain)
        diffuse = gl.render(c, p)[1]
        assert not is_glossy_kernel(gl.kernel_name())
        gl.upload_scene(plain)
        assert np.array_equal(bits(diffuse), bits(gl.render(c, p)[1]))
        bound_upload(gl, replaced, roughness)
        gl.update_transforms(plain)
        gl.update_transforms(replaced)
        assert np.array_equal(bits(got), bits(gl.render(c, p)[1]))
    finally:
        gl.set_builder(T.BUILD_HOST_SAH)


# ---- 7. isolation ---------------------------------------------------------------------------------------------------------------------

def test_glossy_frames_leave_the_other_modes_and_the_gbuffer_alone(gl):
    """test_gpu_nee.py's sequence, with a bound frame between its steps."""
    w, h = 40, 24
    c = cam(w, h)
    scene = scenes.cornell_mirror_scene()
    targets = mirrors(scene)
    p1 = lib.render_params(w, h, 4, 1, seed=3, shade_mode=PATH)
    p2 = lib.render_params(w, h, 4, 2, seed=4, shade_mode=PATH)
    pn = lib.render_params(w, h, 4, 3, seed=5, shade_mode=NEE)

    def sequence(t, with_glossy):
        t.upload_scene(scene)
        out = []
        for step in ("p1", "p1", "gb", "p2", "p1", "gbn"):
            if with_glossy:
                for g in targets:
                    t.set_roughness(g, 0.3)
                t.render(c, pn)
                t.render(c, p2)
                out_bound_gb = t.gbuffer(c, p1)
                for g in targets:
                    t.set_roughness(g, 0.0)
            if step == "gb":
                out.append(t.gbuffer(c, p1))
                if with_glossy:
                    out.append(out_bound_gb)  # (the G-buffer of the bound scene)
                else:
                    out.append(t.gbuffer(c, p1))
            elif step == "gbn":
                out.append(t.gbuffer(c, pn))
            else:
                out.append({"rad": t.render(c, p1 if step == "p1" else p2)[1]})
        return out

    with lib.Tracer(0) as fresh:
        a = sequence(fresh, False)
    b = sequence(gl, True)
    for x, y in zip(a, b):
        for k in x:
            assert np.array_equal(x[k].view(np.uint8), y[k].view(np.uint8)), k


# ---- 8. refusals and errors -----------------------------------------------------------------------------------------------------------

def test_argument_checks_and_refusals(gl):
    w, h = 16, 16
    c = cam(w, h)
    with lib.Tracer(0) as empty:
        with pytest.raises(lib.FireflyError) as e:
            empty.set_roughness(0, 0.3)
        assert e.value.status == T.FF_ERR_NO_SCENE
    scene = scenes.cornell_glass_scene()
    gl.upload_scene(scene)
    kinds = {scene.geometries[i].m_bxdf.contents.m_type: i for i in range(len(scene))}
    for kind in (T.BXDF_DIFFUSE, T.BXDF_EMITTER, T.BXDF_GLASS):
        with pytest.raises(lib.FireflyError) as e:
            gl.set_roughness(kinds[kind], 0.3)
        assert e.value.status == T.FF_ERR_UNSUPPORTED
    for args in ((99, 0.3), (-1, 0.3), (kinds[T.BXDF_MIRROR], -0.1), (kinds[T.BXDF_MIRROR], 1.5), (kinds[T.BXDF_MIRROR], np.nan), (kinds[T.BXDF_MIRROR], np.inf)):
        with pytest.raises(lib.FireflyError) as e:
            gl.set_roughness(*args)
        assert e.value.status == T.FF_ERR_INVALID_ARG
    # SMOOTH refuses while an applied binding exists; NORMAL_DEBUG ignores it; an upload drops the bindings
    pd = lib.render_params(w, h, 1, 1, shade_mode=T.SHADE_NORMAL_DEBUG)
    ps = lib.render_params(w, h, 2, 1, shade_mode=T.SHADE_DIFFUSE_PATH_SMOOTH)
    pp = lib.render_params(w, h, 3, 2, shade_mode=PATH)
    dbg, smooth, plain = gl.render(c, pd), gl.render(c, ps)[1], gl.render(c, pp)[1]
    gl.set_roughness(kinds[T.BXDF_MIRROR], 1.0)
    with pytest.raises(lib.FireflyError) as e:
        gl.render(c, ps)
    assert e.value.status == T.FF_ERR_UNSUPPORTED
    again = gl.render(c, pd)
    assert np.array_equal(bits(dbg[1]), bits(again[1])) and np.array_equal(dbg[0], again[0])
    gl.render(c, pp)
    assert is_glossy_kernel(gl.kernel_name())
    gl.upload_scene(scene)
    assert np.array_equal(bits(smooth), bits(gl.render(c, ps)[1]))
    assert np.array_equal(bits(plain), bits(gl.render(c, pp)[1]))
    assert not gl.kernel_name().startswith("nee_path_kernel")


def test_multi_device_entry_points_refuse():
    w, h = 16, 16
    c = cam(w, h)
    scene = scenes.cornell_mirror_scene()
    with lib.MultiTracer([0, 0]) as m:  # (two states: the scene is compiled once and copied, as on two devices)
        m.upload_scene(scene)
        st = m._lib.ff_multi_state(m._handle, 0)
        m.render(c, lib.render_params(w, h, 2, 1, shade_mode=PATH))
        lib.check(m._lib.ff_set_roughness(st, mirrors(scene)[0], 0.3))
        with pytest.raises(lib.FireflyError) as e:
            m.render(c, lib.render_params(w, h, 2, 1, shade_mode=PATH))
        assert e.value.status == T.FF_ERR_UNSUPPORTED
        # the state itself: its scene came from ff_multi_upload_scene, so it has no light table to render a bound frame with
        rad = np.zeros((h, w, 3), np.float32)
        for mode in (PATH, NEE):
            p = lib.render_params(w, h, 2, 1, shade_mode=mode)
            assert m._lib.ff_render(st, C.byref(c), C.byref(p), None, 0, rad.ctypes.data, 0) == T.FF_ERR_UNSUPPORTED
        m.render(c, lib.render_params(w, h, 2, 1, shade_mode=T.SHADE_NORMAL_DEBUG))
        lib.check(m._lib.ff_set_roughness(st, mirrors(scene)[0], 0.0))
        m.render(c, lib.render_params(w, h, 2, 1, shade_mode=PATH))


def test_distributed_entry_point_refuses():
    """On a one-rank communicator (a tracer of its own, as tests/test_gpu_dist.py sets it up)."""
    if not lib.dist_available():
        pytest.fail("the RCCL library is not loadable: ff_render_distributed cannot be exercised")
    w, h = 16, 16
    c = cam(w, h)
    scene = scenes.cornell_mirror_scene()
    with lib.Tracer(0) as t:
        t.upload_scene(scene)
        t.dist_init(0, 1, lib.dist_unique_id())
        try:
            p = lib.render_params(w, h, 2, 1, shade_mode=PATH)
            plain = t.render_distributed(c, p)[1]
            t.set_roughness(mirrors(scene)[0], 0.3)
            with pytest.raises(lib.FireflyError) as e:
                t.render_distributed(c, p)
            assert e.value.status == T.FF_ERR_UNSUPPORTED
            t.render_distributed(c, lib.render_params(w, h, 1, 1, shade_mode=T.SHADE_NORMAL_DEBUG))
            t.set_roughness(mirrors(scene)[0], 0.0)
            assert np.array_equal(bits(plain), bits(t.render_distributed(c, p)[1]))
        finally:
            t.dist_shutdown()
