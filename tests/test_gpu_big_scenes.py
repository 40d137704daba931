"""The G-buffer and the ray kernels on scenes of more than 32 geometries (tests/big_scenes.py): scenes of exactly 32, 33, 128 and 129
records - either side of both boundaries of csrc/ff_kernels.hip scene_size_class - and the two crowds the suite renders elsewhere.
What the pre-pass stores per pixel (trace_bvh_kernel<false, B, true, BIG, true>, BIG = 1 and 2) is what ff_gbuffer resolves, so every
channel is compared bit for bit with the CPU oracle's intersectRays of each pixel's primary ray; frames and ff_intersect_rays at the
boundary counts equal the brute-force kernels and the oracle; the instantiation each count runs is pinned by name."""
import functools

import numpy as np
import pytest

import big_scenes as B
import texture_ref
from gpupathtracer_amd import lib, scenes
from gpupathtracer_amd import types as T
from gbuffer_ref import oracle_gbuffer
from oracle_lib import oracle_intersect, oracle_render
from test_gpu_dynamic import check_trees
from test_gpu_gbuffer import assert_same_bits
from test_gpu_parity import _random_rays
from test_gpu_texture import expected_albedo

pytestmark = pytest.mark.gpu

W, H = B.W, B.H
F = np.float32


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@functools.lru_cache(maxsize=None)
def _case(name):
    """(scene, camera, params, the oracle's G-buffer): computed once, shared by every test, never written to."""
    scene_fn, cam_fn = B.SCENES[name]
    scene, cam, params = scene_fn(), cam_fn(), lib.render_params(W, H)
    want = oracle_gbuffer(scene, cam, params)
    for v in want.values():
        v.setflags(write=False)
    return scene, cam, params, want


@functools.lru_cache(maxsize=None)
def _moved():
    moved, shelf, picked = B.moved_scene(129)
    want = oracle_gbuffer(moved, B.camera(), lib.render_params(W, H))
    for v in want.values():
        v.setflags(write=False)
    return moved, shelf, picked, want


# ---- a. every channel against the oracle ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(B.SCENES))
def test_every_channel_matches_the_oracle_fresh_and_from_kept_hits(tracer, name):
    """Right after an upload ff_gbuffer runs a pre-pass of its own; after a path frame of the same camera it resolves the hits the
    frame's pre-pass kept.  Both are the oracle's bits."""
    scene, cam, params, want = _case(name)
    tracer.upload_scene(scene)
    assert_same_bits(tracer.gbuffer(cam, params), want, f"{name} fresh")
    _, rad = tracer.render(cam, lib.render_params(W, H, 3, 4, 5, T.TRACE_BVH, T.SHADE_DIFFUSE_PATH))
    assert rad.max() > 0
    assert_same_bits(tracer.gbuffer(cam, params), want, f"{name} kept")


def test_records_in_global_memory_with_the_reference_grid_and_device_buffers(tracer):
    import torch
    scene, cam, params, want = _case("n129")
    tracer.upload_scene(scene)
    # (64 x 48 is whole 16 x 16 tiles: the reference's grid covers the frame, and the launch is sized by it)
    assert_same_bits(tracer.gbuffer(cam, lib.render_params(W, H, grid_mode=T.GRID_REFERENCE_FLOOR)), want, "n129 reference-floor grid")
    dev = {k: torch.zeros(v.shape, dtype=torch.int32 if k == "ids" else torch.float32, device="cuda") for k, v in want.items()}
    tracer.gbuffer_device(cam, params, dev["depth"].data_ptr(), dev["position"].data_ptr(), dev["normal"].data_ptr(), dev["albedo"].data_ptr(),
                          dev["ids"].data_ptr())
    torch.cuda.synchronize()
    assert_same_bits({k: v.cpu().numpy() for k, v in dev.items()}, want, "n129 device buffers")


# ---- b. the boundary counts in every ray kernel ------------------------------------------------------------------------------------------

NAMES = {32: "trace_bvh_kernel<false, 1024, true, 0, false>",  # (the scene has mirrors: the small-scene kernel with the extras)
         33: "trace_bvh_kernel<false, 1024, true, 1, false>", 128: "trace_bvh_kernel<false, 1024, true, 1, false>",
         129: "trace_bvh_kernel<false, 1024, true, 2, false>"}


@pytest.mark.parametrize("n", B.COUNTS)
def test_boundary_count_frames_equal_brute_force_and_the_oracle(tracer, n):
    scene, cam, _, _ = _case(f"n{n}")
    tracer.upload_scene(scene)
    p = lib.render_params(W, H, 4, 2, 7, T.TRACE_BVH, T.SHADE_DIFFUSE_PATH)
    rgb8, rad = tracer.render(cam, p)
    p.trace_mode = T.TRACE_BRUTE_FORCE
    b8, brad = tracer.render(cam, p)
    o8, orad = oracle_render(scene, cam, p, threads=16)
    assert orad.max() > 0
    assert np.array_equal(rgb8, b8) and np.array_equal(bits(rad), bits(brad)), f"{n}: the BVH frame differs from the brute-force frame"
    assert np.array_equal(rgb8, o8), f"{n}: {(rgb8 != o8).any(axis=2).sum()} pixels differ from the oracle in rgb8"
    assert np.array_equal(bits(rad), bits(orad)), f"{n}: {(bits(rad) != bits(orad)).any(axis=2).sum()} pixels differ from the oracle in radiance"


@pytest.mark.parametrize("n", B.COUNTS)
def test_boundary_counts_run_their_size_class(tracer, n):
    scene, cam, _, _ = _case(f"n{n}")
    tracer.upload_scene(scene)
    tracer.set_collect_stats(False)
    tracer.render(cam, lib.render_params(W, H, 2, 1, 3, T.TRACE_BVH, T.SHADE_DIFFUSE_PATH))
    assert tracer.kernel_name() == NAMES[n]


@pytest.mark.parametrize("mode", [T.TRACE_BVH, T.TRACE_BRUTE_FORCE], ids=["bvh", "brute"])
@pytest.mark.parametrize("n", B.COUNTS)
def test_boundary_count_intersect_rays_equal_the_oracle(tracer, n, mode):
    scene, _, _, _ = _case(f"n{n}")
    o, d, exp = _rays(n)
    tracer.upload_scene(scene)
    got = tracer.intersect_rays(o, d, mode)
    assert got["hit"].sum() > 300, "test rays should hit the scene"
    assert np.array_equal(got["hit"], exp["hit"])
    h = exp["hit"] == 1
    assert np.array_equal(got["geom"][h], exp["geom"][h])
    assert np.array_equal(got["tri"][h], exp["tri"][h])
    for f in ("t", "point", "normal"):
        assert np.array_equal(got[f][h].view(np.uint32), exp[f][h].view(np.uint32)), f
    assert (got["geom"][~h] == -1).all() and (got["t"][~h] == 0).all()
    assert len(np.unique(exp["geom"][h])) > 15  # (the rays reach the fill, not the walls alone)


@functools.lru_cache(maxsize=None)
def _rays(n):
    """1500 seeded rays, half from inside the box and half from outside towards it, and the oracle's answer for counted_scene(n)."""
    oi, di = _random_rays(750, 21, inside_box=True)
    oo, do = _random_rays(750, 22, inside_box=False)
    o, d = np.concatenate([oi, oo]), np.concatenate([di, do])
    exp = oracle_intersect(_case(f"n{n}")[0], o, d)
    for a in (o, d, exp):
        a.setflags(write=False)
    return o, d, exp


# ---- c. device-built trees ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("builder", [T.BUILD_GPU_LBVH, T.BUILD_GPU_PLOC], ids=["lbvh", "ploc"])
@pytest.mark.parametrize("n", [33, 129])
def test_device_built_trees_give_the_same_g_buffer(n, builder):
    scene, cam, params, want = _case(f"n{n}")
    with lib.Tracer(0) as t:
        t.set_builder(builder)
        t.upload_scene(scene)
        assert t.build_stats().builder == builder
        assert_same_bits(t.gbuffer(cam, params), want, f"n{n} builder {builder}")
        assert check_trees(t, n) >= 1


# ---- d. one tracer across the classes ---------------------------------------------------------------------------------------------------

def test_one_tracer_across_the_size_classes():
    """32, 129, 33, 128 and 32 again on one state: nothing of the larger scene (a count, an LDS layout, the kept hits of its frame)
    may serve the next."""
    got = []
    with lib.Tracer(0) as t:
        for n in (32, 129, 33, 128, 32):
            scene, cam, params, want = _case(f"n{n}")
            t.upload_scene(scene)
            got.append(t.gbuffer(cam, params))
            assert_same_bits(got[-1], want, f"n{n} after {len(got) - 1} uploads")
            t.render(cam, lib.render_params(W, H, 2, 2, 9, T.TRACE_BVH, T.SHADE_DIFFUSE_PATH))  # (leaves this scene's hits behind)
    assert_same_bits(got[-1], got[0], "32 again")


# ---- e. a moved big scene ------------------------------------------------------------------------------------------------------------------

def test_moved_big_scene(tracer):
    scene, cam, params, before = _case("n129")
    moved, shelf, picked, want = _moved()
    frame = lib.render_params(W, H, 3, 2, 11, T.TRACE_BVH, T.SHADE_DIFFUSE_PATH)
    tracer.upload_scene(scene)
    tracer.render(cam, frame)  # (stored hits of the scene before the move)
    tracer.update_transforms(moved)
    got = tracer.gbuffer(cam, params)
    assert_same_bits(got, want, "moved")
    assert not np.array_equal(bits(got["depth"]), bits(before["depth"]))
    for i in shelf:  # the shelf records are still in view, somewhere else
        m, m0 = want["ids"][..., 0] == i, before["ids"][..., 0] == i
        assert m.sum() >= 4 and not np.array_equal(m, m0), i
    rgb8, rad = tracer.render(cam, frame)
    with lib.Tracer(0) as fresh:
        fresh.upload_scene(moved)
        f8, frad = fresh.render(cam, frame)
    assert np.array_equal(rgb8, f8) and np.array_equal(bits(rad), bits(frad))
    assert_same_bits(tracer.gbuffer(cam, params), want, "moved, from the frame's kept hits")


# ---- f. bound state on a big scene ---------------------------------------------------------------------------------------------------------

def test_texture_and_jitter_on_a_big_scene(tracer):
    """An albedo texture on the shelf quad of index 128 - the first record past what LDS holds - under a pixel jitter: its albedo is
    m_albedo * texel(uv * scale + offset) at the G-buffer's own positions, as tests/test_gpu_texture.py forms it, and every other
    value is the oracle's for the jittered rays, as tests/test_gpu_jitter.py forms them."""
    scene, cam, params, unjittered = _case("n129")
    quad, jitter = 128, (0.3, 0.8)
    texels, flags, scale, offset = scenes.gradient_texture(37, 23), T.TEX_REPEAT, (3.0, 2.0), (0.13, 0.71)
    want = B.oracle_gbuffer_jittered(scene, cam, params, *jitter)
    tracer.upload_scene(scene)
    tid = tracer.create_texture(texels, flags)
    try:
        tracer.set_albedo_texture(quad, tid, scale, offset)
        tracer.set_pixel_jitter(*jitter)
        got = tracer.gbuffer(cam, params)
    finally:
        tracer.set_pixel_jitter(0.0, 0.0)
        tracer.destroy_texture(tid)
    on_quad = want["ids"][..., 0] == quad
    assert on_quad.sum() >= 4
    assert not np.array_equal(bits(want["depth"]), bits(unjittered["depth"]))  # (the jitter does move the rays)
    for k in want:
        sel = ~on_quad if k == "albedo" else np.ones_like(on_quad)
        bad = np.argwhere(bits(got[k])[sel] != bits(want[k])[sel])
        assert bad.size == 0, f"{k}: {len(bad)} values differ from the jittered oracle, first at {bad[:3].tolist()}"
    alb, mask = expected_albedo(scene, got, {quad: (texels, flags, scale, offset)}, {})
    assert np.array_equal(mask, on_quad)
    assert np.array_equal(bits(got["albedo"][mask]), bits(alb[mask])), np.argwhere(np.any(got["albedo"] != alb, -1) & mask)[:5]
    # ... and the same through the float32 restatement of the lookup
    uv = lib.surface_uv(scene, quad, got["position"][mask])
    base = scene.geometries[quad].m_bxdf.contents.m_albedo
    twin = np.array([base.x, base.y, base.z], F) * texture_ref.sample(texels, (uv * np.asarray(scale, F) + np.asarray(offset, F)).astype(F), flags)
    assert np.array_equal(bits(got["albedo"][mask]), bits(twin))
    assert len(np.unique(got["albedo"][mask], axis=0)) > 3  # (a gradient, not one colour)
