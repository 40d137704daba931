"""Per-sample camera rays on the GPU (ff_set_camera_sampling): frames without an active setting stay bit for bit what they were, the
kernel traces exactly the host twin's rays, direct lighting against the float64 reference (tests/camera_ref.py), a surface in the
plane of focus renders as the pinhole's, one off it blurs, the box filter's coverage of an edge pixel, determinism across trace
modes, launches, tiles, strips and progressive frames, isolation from NORMAL_DEBUG and ff_gbuffer, and the refusals."""
import ctypes as C

import numpy as np
import pytest

from gpupathtracer_amd import lib, scenes
from gpupathtracer_amd import types as T
import camera_ref
import nee_ref
from test_gpu_glossy import check_direct

pytestmark = pytest.mark.gpu

NEE, PATH = T.SHADE_DIFFUSE_PATH_NEE, T.SHADE_DIFFUSE_PATH
INSIDE = dict(position=(0.0, 0.0, 2.4), yaw=-90.0, pitch=0.0)
BOX = dict(pixel_filter=T.PIXEL_BOX)
LENS = dict(lens_radius=0.2, focus_distance=5.0)
BOTH = dict(pixel_filter=T.PIXEL_BOX, lens_radius=0.2, focus_distance=5.0)


def cam(w, h, **pose):
    return scenes.posed_camera(w, h, **(pose or INSIDE))


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def is_camera_kernel(name):
    """nee_path_kernel<MODE, BIG, ENV, TEX, GLOSSY, 1>: the instantiations with CAM are the ones named by all six parameters."""
    return name.startswith("nee_path_kernel<") and name.count(",") == 5 and name.endswith(", 1>")


@pytest.fixture
def ct(tracer):
    """The session's tracer, with today's camera, no jitter and no environment before and after."""
    def reset():
        tracer.set_camera_sampling(None)
        tracer.set_pixel_jitter(0.0, 0.0)
        tracer.clear_environment()
    reset()
    yield tracer
    reset()


# ---- 1. nothing set, nothing changes -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["C2", "mirror"])
@pytest.mark.parametrize("mode", [PATH, NEE])
@pytest.mark.parametrize("trace", [T.TRACE_BVH, T.TRACE_BRUTE_FORCE])
@pytest.mark.parametrize("spp", [1, 130])
def test_nothing_set_nothing_changes(ct, name, mode, trace, spp):
    scene = scenes.cornell_wahoo_scene() if name == "C2" else scenes.cornell_mirror_scene()
    w, h = 24, 16
    c = cam(w, h)
    p = lib.render_params(w, h, 4, spp, seed=17, trace_mode=trace, shade_mode=mode)
    # a state no call of the new interface has touched renders the frame twice (a second 1-spp frame from a camera at rest starts
    # from the kept hits: another instantiation, the same bits)
    with lib.Tracer(0) as fresh:
        fresh.upload_scene(scene)
        want = []
        for _ in range(2):
            want.append(fresh.render(c, p) + (fresh.kernel_name(),))
    assert not any(is_camera_kernel(k) for _, _, k in want)
    assert np.array_equal(bits(want[0][1]), bits(want[1][1]))
    ct.upload_scene(scene)
    ct.set_camera_sampling(lib.camera_sampling())
    got = ct.render(c, p)
    assert ct.kernel_name() == want[0][2]
    assert np.array_equal(bits(got[1]), bits(want[0][1])) and np.array_equal(got[0], want[0][0])
    ct.set_camera_sampling(lib.camera_sampling(**BOTH))
    active = ct.render(c, p)[1]
    assert is_camera_kernel(ct.kernel_name()) and not np.array_equal(bits(active), bits(want[0][1]))
    ct.set_camera_sampling(None)
    got = ct.render(c, p)
    assert ct.kernel_name() == want[1][2]
    assert np.array_equal(bits(got[1]), bits(want[1][1])) and np.array_equal(got[0], want[1][0])


# ---- 2. the kernel traces exactly the twin's rays ------------------------------------------------------------------------------------

def emitters_scene():
    """Emitters only, in front of nothing: three emitting planes of distinct colours at different depths and an emitting cube."""
    s = scenes.Scene()
    s.add_plane((-1.5, 0.5, -2.0), (0, 0, 0), (3, 3, 3), scenes.make_bxdf(T.BXDF_EMITTER, emissive=(1.0, 0.2, 0.1), intensity=1.5))
    s.add_plane((1.2, -0.8, 0.0), (0, 0, 0), (2, 2, 2), scenes.make_bxdf(T.BXDF_EMITTER, emissive=(0.1, 0.9, 0.3), intensity=0.7))
    s.add_plane((-0.5, -1.0, 1.5), (10, 25, 5), (1.2, 1.2, 1.2), scenes.make_bxdf(T.BXDF_EMITTER, emissive=(0.2, 0.3, 1.0), intensity=2.25))
    s.add_mesh(scenes.load_mesh("cube"), (0.8, 1.0, 0.5), (20, 30, 0), (0.8, 0.8, 0.8), scenes.make_bxdf(T.BXDF_EMITTER, emissive=(0.9, 0.8, 0.1), intensity=1.1))
    return s.finalize()


EMITTERS_CAM = dict(position=(0.1, 0.2, 5.0), yaw=-92.0, pitch=-3.0)


def expected_emission(tracer, scene, c, sampling, p, jitter):
    """bounces = 1: the twin's rays through ff_intersect_rays, the emission of what they hit, summed in the kernel's order - 64-sample
    blocks sequentially from 0, then the blocks in order - times 1 / spp, all in float32."""
    w, h, spp = p.width, p.height, p.spp
    _, le = nee_ref.emission_of(scene)
    le = np.concatenate([le.astype(np.float32), np.zeros((1, 3), np.float32)])  # (index -1: a miss)
    origins, dirs = camera_ref.frame_rays(c, sampling, w, h, p.seed, spp, jitter=jitter)  # (the jitter the state holds, as in a frame)
    total = np.zeros((h, w, 3), np.float32)
    hits = 0
    for first in range(0, spp, 64):
        block = np.zeros((h, w, 3), np.float32)
        for s in range(first, min(spp, first + 64)):
            got = tracer.intersect_rays(origins[s].reshape(-1, 3), dirs[s].reshape(-1, 3), trace_mode=p.trace_mode)
            g = np.where(np.asarray(got["hit"]) != 0, np.asarray(got["geom"]), -1).reshape(h, w)
            hits += int((g >= 0).sum())
            block = block + le[g]
        total = total + block
    return total * (np.float32(1.0) / np.float32(spp)), hits


@pytest.mark.parametrize("setting", [BOX, LENS, BOTH], ids=["box", "lens", "both"])
@pytest.mark.parametrize("mode", [PATH, NEE])
@pytest.mark.parametrize("trace", [T.TRACE_BVH, T.TRACE_BRUTE_FORCE])
@pytest.mark.parametrize("spp", [1, 4, 130])
def test_the_kernel_traces_the_twins_rays(ct, setting, mode, trace, spp):
    scene = emitters_scene()
    w, h = 48, 36
    c = cam(w, h, **EMITTERS_CAM)
    cs = lib.camera_sampling(**setting)
    p = lib.render_params(w, h, 1, spp, seed=(3 << 32) | 77, trace_mode=trace, shade_mode=mode)
    ct.upload_scene(scene)
    ct.set_pixel_jitter(0.25, 0.5)  # (applied to a CORNER frame, and to none with BOX)
    ct.set_camera_sampling(cs)
    rad = ct.render(c, p)[1]
    assert is_camera_kernel(ct.kernel_name())
    want, hits = expected_emission(ct, scene, c, cs, p, (0.25, 0.5))
    assert 0.1 * w * h * spp < hits < 0.9 * w * h * spp  # (hits and misses both: the emitters cover about a fifth of the view)
    assert np.array_equal(bits(rad), bits(want))


# ---- 3. direct lighting -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["C2", "triangle_lights"])
@pytest.mark.parametrize("spp", [1, 4])
def test_direct_lighting_matches_the_reference(ct, name, spp):
    scene = scenes.cornell_wahoo_scene() if name == "C2" else nee_ref.triangle_light_scene()
    w, h = 64, 48
    c = cam(w, h)
    cs = lib.camera_sampling(T.PIXEL_BOX, 0.05, 3.0)
    params = lib.render_params(w, h, bounces=2, spp=spp, seed=2024, shade_mode=NEE)
    ct.upload_scene(scene)
    ref, hit, excused = camera_ref.direct_lighting(ct, scene, c, cs, params)
    # the reference alone: the rays it cannot decide stay within check_direct's cap for this camera
    assert hit.sum() > 0.9 * w * h and excused[hit].mean() <= 0.05
    ct.set_camera_sampling(cs)
    got = ct.render(c, params)[1].astype(np.float64)
    assert is_camera_kernel(ct.kernel_name())
    check_direct(got, ref, hit, excused)


def test_path_mode_keeps_its_expectation(ct):
    """FF_SHADE_DIFFUSE_PATH under a setting runs the NEE kernel with no light sample: emitter hits keep weight 1, so the image mean
    is the mean of the frames without the setting (test_gpu_nee.py's z-test on the image mean; a box filter moves no energy)."""
    scene = scenes.cornell_wahoo_scene()
    w, h, seeds = 32, 24, 12
    c = cam(w, h)
    ct.upload_scene(scene)
    means = {}
    for on in (False, True):
        ct.set_camera_sampling(lib.camera_sampling(**BOX) if on else None)
        means[on] = np.array([ct.render(c, lib.render_params(w, h, 6, 32, seed=500 + s, shade_mode=PATH))[1].astype(np.float64).mean() for s in range(seeds)])
        assert is_camera_kernel(ct.kernel_name()) == on
    z = abs(means[True].mean() - means[False].mean()) / np.sqrt(means[True].var(ddof=1) / seeds + means[False].var(ddof=1) / seeds)
    print(f"image means {means[False].mean():.5f} {means[True].mean():.5f}, z = {z:.2f}")
    assert means[False].mean() > 0.0 and z < 5.0


# ---- 4-6. one emitting quad facing the camera ------------------------------------------------------------------------------------------

QUAD_W, QUAD_H, QUAD_F = 32, 24, 4.0
QUAD_LE = np.array([2.0, 1.0, 0.5], np.float32)  # (powers of two: sums of equal samples are exact)


def quad_camera():
    return scenes.posed_camera(QUAD_W, QUAD_H, position=(0.0, 0.0, 5.0), yaw=-90.0, pitch=0.0)  # looks down -z: right = +x, up = +y


def plane_points(c, px, py):
    """Where the pinhole ray through pixel-grid point (px, py) meets the plane at depth QUAD_F, in float64 from the camera matrix."""
    m = camera_ref.ray_matrix(c).astype(np.float64)
    far = float(c.m_farClip)
    ndc = np.stack([(np.asarray(px, float) / c.m_screenWidth) * 2 - 1, 1 - (np.asarray(py, float) / c.m_screenHeight) * 2], -1)
    v = np.concatenate([ndc * far, np.full(ndc.shape[:-1] + (2,), far)], -1)
    pos = camera_ref.vec(c.m_position).astype(np.float64)
    d = (v @ m)[..., :3] - pos
    fwd = camera_ref.vec(c.m_forward).astype(np.float64)
    return pos + d * (QUAD_F / (d @ fwd))[..., None]


def quad_scene():
    """A quad in the plane at depth QUAD_F whose edges fall at pixel-grid x = 10.5 and 20.4 and y = 6.5 and 17.5: half of pixel
    column 10 and 0.4 of column 20 are covered.  Returns (scene, (x0, x1, y_bottom, y_top) of the float32 quad in world units)."""
    c = quad_camera()
    corners = plane_points(c, [10.5, 20.4], [17.5, 6.5])
    x0, x1, y0, y1 = corners[0, 0], corners[1, 0], corners[0, 1], corners[1, 1]
    pos = np.array([(x0 + x1) / 2, (y0 + y1) / 2, 5.0 - QUAD_F], np.float32)
    scl = np.array([x1 - x0, y1 - y0, 1.0], np.float32)
    s = scenes.Scene()
    s.add_plane(tuple(float(v) for v in pos), (0, 0, 0), tuple(float(v) for v in scl),
                scenes.make_bxdf(T.BXDF_EMITTER, emissive=(1.0, 0.5, 0.25), intensity=2.0))
    edges = (float(pos[0]) - float(scl[0]) / 2, float(pos[0]) + float(scl[0]) / 2, float(pos[1]) - float(scl[1]) / 2, float(pos[1]) + float(scl[1]) / 2)
    return s.finalize(), edges


def test_in_focus_is_the_pinhole(ct):
    scene, (x0, x1, y0, y1) = quad_scene()
    c = quad_camera()
    w, h, spp = QUAD_W, QUAD_H, 4
    cs = lib.camera_sampling(T.PIXEL_CORNER, 0.3, QUAD_F)
    # precondition, in float64 from the twin's rays: no ray meets the quad's plane within 1e-3 of an edge
    o, d = (a.astype(np.float64) for a in camera_ref.frame_rays(c, cs, w, h, 9, spp))
    at = o + d * ((5.0 - QUAD_F - o[..., 2]) / d[..., 2])[..., None]
    for edge, axis in ((x0, 0), (x1, 0), (y0, 1), (y1, 1)):
        assert np.abs(at[..., axis] - edge).min() > 1e-3
    ct.upload_scene(scene)
    for mode in (PATH, NEE):
        p = lib.render_params(w, h, 1, spp, seed=9, shade_mode=mode)
        ct.set_camera_sampling(None)
        pinhole = ct.render(c, p)
        ct.set_camera_sampling(cs)
        lens = ct.render(c, p)
        assert is_camera_kernel(ct.kernel_name())
        assert np.array_equal(bits(lens[1]), bits(pinhole[1])) and np.array_equal(lens[0], pinhole[0])
        lit = np.all(pinhole[1] == QUAD_LE, -1)
        assert lit.sum() == 10 * 11 and np.all(pinhole[1][~lit] == 0.0)


def test_out_of_focus_blurs(ct):
    scene, _ = quad_scene()
    c = quad_camera()
    p = lib.render_params(QUAD_W, QUAD_H, 1, 130, seed=9, shade_mode=NEE)
    ct.upload_scene(scene)

    def partial(rad):
        return np.all((rad > 0.0) & (rad < QUAD_LE), -1)

    assert not partial(ct.render(c, p)[1]).any()
    ct.set_camera_sampling(lib.camera_sampling(T.PIXEL_CORNER, 0.3, QUAD_F / 2))
    rad = ct.render(c, p)[1]
    assert partial(rad).sum() > 20
    assert np.all(rad[12, 15] == QUAD_LE) and np.all(rad[0, 0] == 0.0)  # (the blur is an edge's, a few pixels wide)


def test_box_filter_covers_an_edge_pixel_by_its_fraction(ct):
    scene, (x0, x1, y0, y1) = quad_scene()
    c = quad_camera()
    w, h, spp = QUAD_W, QUAD_H, 1024
    ct.upload_scene(scene)
    ct.set_camera_sampling(lib.camera_sampling(**BOX))
    rad = ct.render(c, lib.render_params(w, h, 1, spp, seed=4, shade_mode=NEE))[1].astype(np.float64)
    grid = plane_points(c, np.arange(w + 1), np.zeros(w + 1))[:, 0]  # world x of the pixel columns' bounds (affine in the pixel index)
    for col, edge, covered_right in ((10, x0, True), (20, x1, False)):
        a = (grid[col + 1] - edge) / (grid[col + 1] - grid[col])
        a = a if covered_right else 1.0 - a
        assert 0.25 <= a <= 0.75
        for row in range(7, 17):  # (rows the quad covers fully)
            assert np.all(np.abs(rad[row, col] - a * QUAD_LE) <= 5 * np.sqrt(a * (1 - a) / spp) * QUAD_LE), (col, row, a, rad[row, col])
    assert np.all(rad[7:17, 11:20] == QUAD_LE)
    outside = np.ones((h, w), bool)
    outside[6:18, 10:21] = False
    assert np.all(rad[outside] == 0.0)


# ---- 7. invariances -----------------------------------------------------------------------------------------------------------------------

MIRROR_FLOOR, MIRROR_CUBE, MIRROR_BACK = 3, 1, 2  # geometry indices in scenes.cornell_mirror_scene


def bind_everything(t, scene, texture):
    t.upload_scene(scene)
    t.set_albedo_texture(MIRROR_FLOOR, texture, scale=(3.0, 2.0))
    t.set_roughness(MIRROR_CUBE, 0.3)
    t.set_roughness(MIRROR_BACK, 0.2)


@pytest.fixture
def loaded(ct):
    """Lens and box filter, an environment, a texture and rough mirrors all bound."""
    rng = np.random.default_rng(2)
    texture = ct.create_texture(rng.uniform(0.2, 1.0, (8, 8, 3)).astype(np.float32))
    scene = scenes.cornell_mirror_scene()
    env = np.full((8, 16, 3), 0.3, np.float32)
    env[2, 5] = (40.0, 36.0, 28.0)
    bind_everything(ct, scene, texture)
    ct.set_environment(env, 1.0, 20.0)
    ct.set_camera_sampling(lib.camera_sampling(T.PIXEL_BOX, 0.08, 2.5))
    yield ct, scene, texture
    ct.destroy_texture(texture)


def test_invariances(loaded):
    t, scene, texture = loaded
    w, h = 40, 30
    c = cam(w, h)
    p = lib.render_params(w, h, 4, 130, seed=8, shade_mode=NEE)
    full = t.render(c, p)[1]
    assert full.max() > 0.0 and t.kernel_name() == "nee_path_kernel<1, 0, 1, 1, 1, 1>"
    assert np.array_equal(bits(full), bits(t.render(c, p)[1]))
    brute = t.render(c, lib.render_params(w, h, 4, 130, seed=8, shade_mode=NEE, trace_mode=T.TRACE_BRUTE_FORCE))[1]
    assert np.array_equal(bits(full), bits(brute)) and t.kernel_name() == "nee_path_kernel<0, 0, 1, 1, 1, 1>"
    split = t.render(c, lib.render_params(w, h, 4, 130, seed=8, shade_mode=NEE, spp_per_launch=64))[1]
    assert np.array_equal(bits(full), bits(split))
    for (x0, y0, tw, th) in ((0, 0, 16, 8), (13, 7, 20, 17), (36, 25, 4, 5)):
        tile = t.render_tile(c, p, x0, y0, tw, th)[1]
        assert np.array_equal(bits(tile), bits(full[y0:y0 + th, x0:x0 + tw])), (x0, y0)
    strip_rows, parts = 3, 3
    for part in range(parts):
        _, srad = t.render_strips(c, p, strip_rows, part, parts)
        rows = [y for y in range(h) if (y // strip_rows) % parts == part]
        assert np.array_equal(bits(srad), bits(full[rows])), part
    # the setting survives an upload (which drops the scene's bindings) and a transform update
    bind_everything(t, scene, texture)
    assert np.array_equal(bits(full), bits(t.render(c, p)[1]))
    t.update_transforms(scene)
    assert np.array_equal(bits(full), bits(t.render(c, p)[1]))


def test_progressive_is_the_mean_of_its_frames(loaded):
    t, _, _ = loaded
    w, h = 40, 30
    c = cam(w, h)
    frames, acc = [], None
    for i in range(3):
        frames.append(t.render(c, lib.render_params(w, h, 4, 130, seed=300 + i, shade_mode=NEE))[1])
        _, mean = t.render_progressive(c, lib.render_params(w, h, 4, 130, seed=300, shade_mode=NEE), i)
        acc = frames[0].copy() if i == 0 else acc + frames[i]
        assert np.array_equal(bits(mean), bits(acc * np.float32(1.0 / (i + 1))))


# ---- 8. leaves the rest alone --------------------------------------------------------------------------------------------------------------

def test_normal_debug_the_gbuffer_and_the_ray_count(ct):
    w, h = 40, 24
    c = cam(w, h)
    scene = scenes.cornell_wahoo_scene()
    pd = lib.render_params(w, h, 1, 1, shade_mode=T.SHADE_NORMAL_DEBUG)
    ct.upload_scene(scene)
    ct.set_pixel_jitter(0.25, 0.75)
    dbg, gb = ct.render(c, pd), ct.gbuffer(c, pd)
    ct.set_camera_sampling(lib.camera_sampling(**BOTH))
    again, gb2 = ct.render(c, pd), ct.gbuffer(c, pd)
    assert not ct.kernel_name().startswith("nee_path_kernel")
    assert np.array_equal(bits(dbg[1]), bits(again[1])) and np.array_equal(dbg[0], again[0])
    assert sorted(gb) == sorted(gb2) and len(gb) == 5
    for k in gb:
        assert np.array_equal(gb[k].view(np.uint8), gb2[k].view(np.uint8)), k
    for mode in (PATH, NEE):
        for spp in (1, 4, 130):
            ct.render(c, lib.render_params(w, h, 1, spp, seed=2, shade_mode=mode))
            assert ct.stats().rays_traced == w * h * spp


# ---- 9. refusals ------------------------------------------------------------------------------------------------------------------------------

def test_invalid_settings_name_the_field(ct):
    def make(**kw):
        cs = lib.camera_sampling()
        for k, v in kw.items():
            setattr(cs, k, v)
        return cs
    ct.set_camera_sampling(lib.camera_sampling(**BOTH))
    for cs, field in ((make(pixel_filter=2), "pixel_filter"), (make(lens_radius=-0.5), "lens_radius"), (make(lens_radius=float("nan")), "lens_radius"),
                      (make(lens_radius=float("inf")), "lens_radius"), (make(focus_distance=float("nan")), "focus_distance"),
                      (make(focus_distance=float("inf")), "focus_distance"), (make(lens_radius=0.1, focus_distance=0.0), "focus_distance"),
                      (make(lens_radius=0.1, focus_distance=-1.0), "focus_distance"), (make(reserved=1), "reserved")):
        with pytest.raises(lib.FireflyError) as e:
            ct.set_camera_sampling(cs)
        assert e.value.status == T.FF_ERR_INVALID_ARG and field in e.value.message, field
    # a refused setting replaces nothing
    w, h = 16, 16
    ct.upload_scene(scenes.cornell_wahoo_scene())
    ct.render(cam(w, h), lib.render_params(w, h, 2, 1, shade_mode=PATH))
    assert is_camera_kernel(ct.kernel_name())
    assert lib.load().ff_set_camera_sampling(None, None) == T.FF_ERR_INVALID_ARG


def test_smooth_mode_refuses(ct):
    w, h = 16, 16
    c = cam(w, h)
    ct.upload_scene(scenes.cornell_wahoo_scene())
    ps = lib.render_params(w, h, 2, 1, shade_mode=T.SHADE_DIFFUSE_PATH_SMOOTH)
    smooth = ct.render(c, ps)[1]
    for setting in (BOX, LENS):
        ct.set_camera_sampling(lib.camera_sampling(**setting))
        with pytest.raises(lib.FireflyError) as e:
            ct.render(c, ps)
        assert e.value.status == T.FF_ERR_UNSUPPORTED
    ct.set_camera_sampling(None)
    assert np.array_equal(bits(smooth), bits(ct.render(c, ps)[1]))


def test_multi_device_entry_points_refuse():
    w, h = 16, 16
    c = cam(w, h)
    scene = scenes.cornell_mirror_scene()
    cs = lib.camera_sampling(**BOTH)
    with lib.MultiTracer([0, 0]) as m:  # (two states: the scene is compiled once and copied, as on two devices)
        m.upload_scene(scene)
        st = m._lib.ff_multi_state(m._handle, 0)
        m.render(c, lib.render_params(w, h, 2, 1, shade_mode=PATH))
        lib.check(m._lib.ff_set_camera_sampling(st, C.byref(cs)))
        with pytest.raises(lib.FireflyError) as e:
            m.render(c, lib.render_params(w, h, 2, 1, shade_mode=PATH))
        assert e.value.status == T.FF_ERR_UNSUPPORTED
        # the state itself: its scene came from ff_multi_upload_scene, so it has no light table to render such a frame with
        rad = np.zeros((h, w, 3), np.float32)
        for mode in (PATH, NEE):
            p = lib.render_params(w, h, 2, 1, shade_mode=mode)
            assert m._lib.ff_render(st, C.byref(c), C.byref(p), None, 0, rad.ctypes.data, 0) == T.FF_ERR_UNSUPPORTED
        m.render(c, lib.render_params(w, h, 2, 1, shade_mode=T.SHADE_NORMAL_DEBUG))
        lib.check(m._lib.ff_set_camera_sampling(st, None))
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
            t.set_camera_sampling(lib.camera_sampling(**BOTH))
            with pytest.raises(lib.FireflyError) as e:
                t.render_distributed(c, p)
            assert e.value.status == T.FF_ERR_UNSUPPORTED
            t.render_distributed(c, lib.render_params(w, h, 1, 1, shade_mode=T.SHADE_NORMAL_DEBUG))
            t.set_camera_sampling(None)
            assert np.array_equal(bits(plain), bits(t.render_distributed(c, p)[1]))
        finally:
            t.dist_shutdown()
