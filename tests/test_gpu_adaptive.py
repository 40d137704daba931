"""ff_render_adaptive on the GPU: the error kernel bit for bit against the host twin on the planted sizes; threshold 0 and +inf against
ff_render_progressive; the mixed scene (tests/adaptive_cases.py) in both path modes against the restatement's driver
(tests/adaptive_ref.py) - over the CPU oracle in the path mode, over Tracer.render_tile with next-event estimation - bit for bit in
passes, errors, sums, radiance and rgb8; the neighbour guard; the state reset per call."""
import numpy as np
import pytest

from gpupathtracer_amd import lib
from gpupathtracer_amd import types as T
import adaptive_ref as R
from adaptive_cases import (MIX_H, MIX_MAX, MIX_MIN, MIX_SEED, MIX_SPP, MIX_THRESHOLD, MIX_THRESHOLD_NEE, MIX_TILE, MIX_W, PASS_COUNTS, SIZE_IDS, SIZES, CachedRender, assert_mixed,
                            mix_adaptive, mix_camera, mix_params, mix_scene, oracle_drive, planted_sums, wide_sums)

pytestmark = pytest.mark.gpu

F = np.float32
PATH, NEE = T.SHADE_DIFFUSE_PATH, T.SHADE_DIFFUSE_PATH_NEE
GUARD = T.ADAPTIVE_GUARD_NEIGHBOURS


def same_bits(a, b):
    return np.array_equal(R.bits(a), R.bits(b))


@pytest.mark.parametrize("w,h,tile", SIZES, ids=SIZE_IDS)
def test_error_kernel_equals_the_twin_bit_for_bit(tracer, w, h, tile):
    for n in PASS_COUNTS:
        total, even = planted_sums(w, h, n)
        assert same_bits(tracer.adaptive_tile_error(total, even, tile, n), lib.adaptive_tile_error_host(total, even, tile, n)), n
    total, even = wide_sums(w, h)  # (sums whose rounding depends on the order of the adds)
    total[0, 0, 0] = np.inf
    got = tracer.adaptive_tile_error(total, even, tile, 2)
    assert same_bits(got, lib.adaptive_tile_error_host(total, even, tile, 2)) and np.isnan(got[0, 0])


def progressive(tracer, cam, params, frames):
    for k in range(frames):
        out = tracer.render_progressive(cam, params, k)
    return out


def test_threshold_zero_is_the_progressive_frame(tracer):
    tracer.upload_scene(mix_scene())
    cam, params = mix_camera(), mix_params()
    exp_rgb8, exp_rad = progressive(tracer, cam, params, 4)
    # a progressive sequence started before the call continues after it
    other = mix_params(seed=99)
    tracer.render_progressive(cam, other, 0)
    tracer.render_progressive(cam, other, 1)
    rgb8, rad, passes, info = tracer.render_adaptive(cam, params, mix_adaptive(threshold=0.0, max_passes=4))
    assert same_bits(rad, exp_rad) and np.array_equal(rgb8, exp_rgb8) and exp_rad.max() > 0
    assert (passes == 4).all() and info.rectangles == 4 and info.passes_run == 4 and info.tiles == 9 and info.tiles_stopped_early == 0
    assert info.samples == 4 * MIX_W * MIX_H * MIX_SPP
    third = tracer.render_progressive(cam, other, 2)
    exp_third = progressive(tracer, cam, other, 3)
    assert same_bits(third[1], exp_third[1]) and np.array_equal(third[0], exp_third[0])


def test_threshold_infinity_stops_at_min_passes(tracer):
    tracer.upload_scene(mix_scene())
    cam, params = mix_camera(), mix_params()
    exp_rgb8, exp_rad = progressive(tracer, cam, params, 2)
    rgb8, rad, passes, info = tracer.render_adaptive(cam, params, mix_adaptive(threshold=float("inf")))
    assert same_bits(rad, exp_rad) and np.array_equal(rgb8, exp_rgb8)
    assert (passes == 2).all() and info.rectangles == 2 and info.passes_run == 2 and info.tiles_stopped_early == 9


def tile_frames(tracer, cam, shade):
    """Whole frames by seed through Tracer.render_tile (the reference of the NEE mode, which the oracle does not render)."""
    return CachedRender(lambda seed: tracer.render_tile(cam, mix_params(shade, seed), 0, 0, MIX_W, MIX_H)[1])


def check_against(tracer, ref, got, tile=MIX_TILE, w=MIX_W, h=MIX_H):
    rgb8, rad, passes, info = got
    state = tracer.adaptive_state(w, h, tile)
    assert np.array_equal(state["tile_passes"], ref["tile_passes"]), (state["tile_passes"], ref["tile_passes"])
    assert np.array_equal(passes, ref["passes"])
    assert same_bits(state["tile_error"], ref["tile_error"]), (state["tile_error"], ref["tile_error"])
    assert same_bits(state["sum"], ref["sum"]) and same_bits(state["sum_even"], ref["sum_even"])
    assert same_bits(rad, ref["radiance"]) and np.array_equal(rgb8, ref["rgb8"])
    assert info.rectangles == ref["rectangles"] and info.passes_run == ref["passes_run"] and info.samples == ref["pixels_rendered"] * MIX_SPP
    assert info.tiles_stopped_early == int((ref["tile_passes"] < MIX_MAX).sum())
    assert F(info.max_tile_error) == ref["tile_error"].max()


@pytest.mark.parametrize("shade", [PATH, NEE], ids=["path", "nee"])
def test_the_mixed_scene_equals_the_reference_driver(tracer, shade):
    tracer.upload_scene(mix_scene())
    cam = mix_camera()
    threshold = MIX_THRESHOLD if shade == PATH else MIX_THRESHOLD_NEE
    got = tracer.render_adaptive(cam, mix_params(shade), mix_adaptive(threshold=threshold))
    frames = tile_frames(tracer, cam, shade)
    if shade == PATH:
        ref = oracle_drive()
    else:
        ref = R.drive(frames, MIX_W, MIX_H, MIX_SEED, MIX_TILE, MIX_MIN, MIX_MAX, MIX_THRESHOLD_NEE)
    n_t = ref["tile_passes"]
    print("tile passes\n", tracer.adaptive_state(MIX_W, MIX_H, MIX_TILE)["tile_passes"], "\nreference\n", n_t)
    for c in ref["checks"]:
        print("check", c["n"], "\n", c["error"])
    check_against(tracer, ref, got)
    assert_mixed(got[2])  # (in the NEE mode the mix is a fact about the GPU's own frames)
    # every tile's pixels are the mean of render_tile(seed + k), k < n_t
    for ty in range(n_t.shape[0]):
        for tx in range(n_t.shape[1]):
            x0, y0, x1, y1 = R.tile_box(MIX_W, MIX_H, MIX_TILE, tx, ty)
            total = None
            for k in range(int(n_t[ty, tx])):
                f = frames(MIX_SEED + k, x0, y0, x1 - x0, y1 - y0)
                total = f.copy() if total is None else total + f
            assert same_bits(got[1][y0:y1, x0:x1], total * (F(1.0) / F(n_t[ty, tx]))), (tx, ty)


def test_one_tile_really_is_render_tile(tracer):
    """CachedRender cuts rectangles out of whole frames; this holds one of the reference's rectangles against a render_tile of
    exactly that window."""
    tracer.upload_scene(mix_scene())
    cam = mix_camera()
    for shade in (PATH, NEE):
        whole = tracer.render_tile(cam, mix_params(shade, MIX_SEED + 3), 0, 0, MIX_W, MIX_H)[1]
        part = tracer.render_tile(cam, mix_params(shade, MIX_SEED + 3), 16, 32, 32, 8)[1]
        assert same_bits(part, whole[32:40, 16:48])


def test_the_neighbour_guard(tracer):
    tracer.upload_scene(mix_scene())
    cam, params = mix_camera(), mix_params()
    plain = tracer.render_adaptive(cam, params, mix_adaptive())[2]
    got = tracer.render_adaptive(cam, params, mix_adaptive(flags=GUARD))
    ref = oracle_drive(guard=True)
    check_against(tracer, ref, got)
    assert (got[2] >= plain).all() and (got[2] > plain).any()
    grid = ref["tile_passes"].shape
    state = tracer.adaptive_state(MIX_W, MIX_H, MIX_TILE)
    for c in ref["checks"]:
        with np.errstate(invalid="ignore"):
            over = c["active_before"] & ~(c["error"] < F(MIX_THRESHOLD))
        for ty, tx in zip(*np.nonzero(c["stopped"])):
            assert state["tile_passes"][ty, tx] == c["n"]
            assert not over[ty, tx] and not any(over[q] for q in R.neighbours(*grid, ty, tx))


def test_two_calls_agree_and_another_size_reallocates(tracer):
    tracer.upload_scene(mix_scene())
    cam, params = mix_camera(), mix_params(NEE)
    first = tracer.render_adaptive(cam, params, mix_adaptive(threshold=MIX_THRESHOLD_NEE))
    assert_mixed(first[2])
    state1 = tracer.adaptive_state(MIX_W, MIX_H, MIX_TILE)
    # another size and tile in between (larger: the buffers grow), then the first again
    w2, h2 = 100, 70
    from gpupathtracer_amd import scenes
    cam2 = scenes.posed_camera(w2, h2, position=(0.0, 0.5, 9.0), yaw=-90.0, pitch=8.0)
    p2 = lib.render_params(w2, h2, 3, 1, 5, shade_mode=NEE)
    big = tracer.render_adaptive(cam2, p2, lib.adaptive_params(tile=32, min_passes=2, max_passes=4, threshold=MIX_THRESHOLD))
    assert big[2].shape == (h2, w2) and big[3].tiles == 4 * 3 and np.isfinite(big[1]).all() and big[1].max() > 0
    frames2 = CachedRender(lambda seed: tracer.render_tile(cam2, lib.render_params(w2, h2, 3, 1, seed, shade_mode=NEE), 0, 0, w2, h2)[1])
    ref2 = R.drive(frames2, w2, h2, 5, 32, 2, 4, MIX_THRESHOLD)
    assert same_bits(big[1], ref2["radiance"]) and np.array_equal(big[2], ref2["passes"])
    second = tracer.render_adaptive(cam, params, mix_adaptive(threshold=MIX_THRESHOLD_NEE))
    state2 = tracer.adaptive_state(MIX_W, MIX_H, MIX_TILE)
    for a, b in zip(first[:3], second[:3]):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
    for key in state1:
        assert np.array_equal(state1[key].view(np.uint8), state2[key].view(np.uint8)), key
    for name, _ in T.FfAdaptiveInfo._fields_:
        assert getattr(first[3], name) == getattr(second[3], name), name
