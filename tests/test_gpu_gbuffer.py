"""ff_gbuffer on the GPU: every channel bit for bit against the CPU oracle's intersectRays of each pixel's primary ray, its
independence of everything but camera, scene, size and grid, the stored primary hits it reads, and that it leaves the frames
around it exactly as they were."""
import functools

import numpy as np
import pytest

from gpupathtracer_amd import lib, scenes
from gpupathtracer_amd import types as T
from gbuffer_ref import oracle_gbuffer
from oracle_lib import oracle_render

pytestmark = pytest.mark.gpu

W, H = 160, 90


def c2(w=W, h=H):
    return scenes.posed_camera(w, h, position=(0.0, 0.0, 2.4), yaw=-90.0, pitch=0.0)


def oblique(w=W, h=H):
    return scenes.posed_camera(w, h, position=(7.0, 3.0, 9.0), yaw=-128.0, pitch=-14.0)


CASES = {
    "wahoo_c2": (scenes.cornell_wahoo_scene, c2, lambda: lib.render_params(W, H)),
    "wahoo_default_camera": (scenes.cornell_wahoo_scene, lambda: scenes.default_camera(W, H), lambda: lib.render_params(W, H)),
    "spheres_c2": (scenes.cornell_spheres_scene, c2, lambda: lib.render_params(W, H)),
    "glass_c2": (scenes.cornell_glass_scene, c2, lambda: lib.render_params(W, H)),
    "mirror_c2": (scenes.cornell_mirror_scene, c2, lambda: lib.render_params(W, H)),
    "blooper_oblique": (scenes.blooper_scene, oblique, lambda: lib.render_params(W, H)),
    "sphere_floor_grid_200x150": (lambda: scenes.reference_scene(scenes.load_mesh("sphere")), lambda: oblique(200, 150),
                                  lambda: lib.render_params(200, 150, grid_mode=T.GRID_REFERENCE_FLOOR)),
}


@functools.lru_cache(maxsize=None)
def _case(name):
    scene_fn, cam_fn, params_fn = CASES[name]
    scene, cam, params = scene_fn(), cam_fn(), params_fn()
    return scene, cam, params, oracle_gbuffer(scene, cam, params)


def assert_same_bits(got, want, what=""):
    assert set(got) == set(want)
    for k in want:
        assert got[k].shape == want[k].shape, (what, k)
        g, w = got[k].view(np.uint32), want[k].view(np.uint32)
        bad = np.argwhere(g != w)
        assert bad.size == 0, f"{what} {k}: {len(bad)} values differ, first at {bad[:3].tolist()}"


@pytest.mark.parametrize("name", sorted(CASES))
def test_every_channel_matches_the_oracle(tracer, name):
    scene, cam, params, want = _case(name)
    tracer.upload_scene(scene)
    got = tracer.gbuffer(cam, params)
    assert_same_bits(got, want, name)
    ids = want["ids"]
    assert (ids[..., 0] >= 0).any()
    if name == "wahoo_default_camera":
        assert (ids[..., 0] < 0).mean() > 0.5  # mostly misses
    if name == "glass_c2":
        assert {T.BXDF_GLASS, T.BXDF_MIRROR, T.BXDF_DIFFUSE} <= set(np.unique(ids[..., 2]).tolist())
    if name == "sphere_floor_grid_200x150":
        assert (ids[144:, :, 0] == -1).all() and (got["depth"][144:] == 0).all()


def test_device_built_tree_gives_the_same_g_buffer():
    scene, cam, params, want = _case("wahoo_c2")
    with lib.Tracer(0) as t:
        t.set_builder(T.BUILD_GPU_LBVH)
        t.upload_scene(scene)
        assert_same_bits(t.gbuffer(cam, params), want, "lbvh")


def test_only_camera_scene_size_and_grid_matter(tracer):
    scene, cam, base, want = _case("wahoo_c2")
    tracer.upload_scene(scene)
    variants = []
    for shade in (T.SHADE_NORMAL_DEBUG, T.SHADE_DIFFUSE_PATH, T.SHADE_DIFFUSE_PATH_SMOOTH):
        for trace in (T.TRACE_BVH, T.TRACE_BRUTE_FORCE):
            variants.append(lib.render_params(W, H, 1, 1, 1234, trace, shade))
    variants += [lib.render_params(W, H, 8, 64, 99), lib.render_params(W, H, 3, 1000, 7, spp_per_launch=128), lib.render_params(W, H, 255, 3, 2**40 + 5)]
    for p in variants:
        assert_same_bits(tracer.gbuffer(cam, p), want, f"spp {p.spp} bounces {p.bounces} trace {p.trace_mode} shade {p.shade_mode}")


def test_host_and_device_buffers_agree(tracer):
    import torch
    scene, cam, params, want = _case("spheres_c2")
    tracer.upload_scene(scene)
    dev = {k: torch.zeros(v.shape, dtype=torch.int32 if k == "ids" else torch.float32, device="cuda") for k, v in want.items()}
    tracer.gbuffer_device(cam, params, dev["depth"].data_ptr(), dev["position"].data_ptr(), dev["normal"].data_ptr(), dev["albedo"].data_ptr(),
                          dev["ids"].data_ptr())
    torch.cuda.synchronize()
    assert_same_bits({k: v.cpu().numpy() for k, v in dev.items()}, want, "device")
    # any buffer may be left out
    only = torch.zeros(want["normal"].shape, dtype=torch.float32, device="cuda")
    tracer.gbuffer_device(cam, params, normal_ptr=only.data_ptr())
    assert np.array_equal(only.cpu().numpy().view(np.uint32), want["normal"].view(np.uint32))


@pytest.mark.parametrize("shade", [T.SHADE_DIFFUSE_PATH, T.SHADE_DIFFUSE_PATH_SMOOTH])
def test_stored_primary_hits_give_the_same_answer(shade):
    """After a frame of the same camera the call resolves the frame's stored hits (a SMOOTH frame's hold the interpolated normal);
    right after an upload, which drops them, it traces its own.  Both equal the oracle."""
    scene, cam, _, want = _case("wahoo_c2")
    with lib.Tracer(0) as t:
        t.upload_scene(scene)
        t.render(cam, lib.render_params(W, H, 4, 3, 5, T.TRACE_BVH, shade))
        assert_same_bits(t.gbuffer(cam, lib.render_params(W, H)), want, "kept")
        t.upload_scene(scene)
        assert_same_bits(t.gbuffer(cam, lib.render_params(W, H)), want, "fresh")


def test_moved_scene_is_reflected(tracer):
    scene, cam, params, _ = _case("wahoo_c2")
    tracer.upload_scene(scene)
    tracer.render(cam, lib.render_params(W, H, 2, 2, 1))  # (stored hits of the old scene)
    moved = scenes.Scene()
    moved.add_mesh(scenes.load_mesh("wahoo"), (0.4, -2.4, 0.3), (0, 25, 0), (0.35, 0.2, 0.28), scenes.make_bxdf(T.BXDF_DIFFUSE, albedo=(0.2, 0.9, 0)))
    moved.add_mesh(scenes.load_mesh("cube"), (1.2, -2.0, 0.6), (0, 10, 0), (1, 1.5, 1), scenes.make_bxdf(T.BXDF_MIRROR, specular=(0.7, 0.8, 0.9)))
    scenes._box(moved).finalize()
    tracer.update_transforms(moved)
    assert_same_bits(tracer.gbuffer(cam, params), oracle_gbuffer(moved, cam, params), "moved")


def _frames(interleave):
    """The sequence of the issue: 1 spp twice at rest, 64 spp, a new camera, 1 spp, progressive frames 0-3."""
    scene = scenes.cornell_wahoo_scene()
    cam_a, cam_b = c2(), oblique()
    out = []
    with lib.Tracer(0) as t:
        t.upload_scene(scene)

        def g(cam):
            if interleave:
                t.gbuffer(cam, lib.render_params(W, H))

        def frame(name, cam, p):
            g(cam)
            rgb8, rad = t.render(cam, p)
            st = t.stats()
            out.append((name, rgb8, rad.view(np.uint32).copy(), st.rays_traced, st.rays_answered, st.rays_cut_short))
            g(cam)
            after = t.stats()  # (not a frame: the statistics still describe the render)
            assert (after.rays_traced, after.rays_answered, after.kernel_launches, after.kernel_ms) == (st.rays_traced, st.rays_answered,
                                                                                                        st.kernel_launches, st.kernel_ms), name

        frame("1 spp", cam_a, lib.render_params(W, H, 8, 1, 5))
        frame("1 spp at rest", cam_a, lib.render_params(W, H, 8, 1, 6))
        frame("64 spp", cam_a, lib.render_params(W, H, 8, 64, 7))
        frame("new camera", cam_b, lib.render_params(W, H, 8, 1, 8))
        frame("new camera at rest", cam_b, lib.render_params(W, H, 8, 1, 9))
        for f in range(4):
            g(cam_a)
            rgb8, rad = t.render_progressive(cam_a, lib.render_params(W, H, 8, 1, 11), f)
            st = t.stats()
            out.append((f"progressive {f}", rgb8, rad.view(np.uint32).copy(), st.rays_traced, st.rays_answered, st.rays_cut_short))
    return out


def test_g_buffer_calls_leave_the_frames_around_them_as_they_were():
    plain, mixed = _frames(False), _frames(True)
    for a, b in zip(plain, mixed):
        assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]), a[0]
        assert a[3:] == b[3:], (a[0], a[3:], b[3:])
    scene = scenes.cornell_wahoo_scene()
    rgb8, rad = oracle_render(scene, c2(), lib.render_params(W, H, 8, 1, 5), threads=8)
    assert np.array_equal(mixed[0][1], rgb8)
    got = mixed[0][2].view(np.float32).astype(np.float64)
    assert np.linalg.norm(got - rad) <= 1e-4 * np.linalg.norm(rad.astype(np.float64))  # (the suite's parity bound, __graft_entry__.smoke)
