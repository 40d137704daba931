"""Which instantiation a frame runs (csrc/ff_kernels.hip launch_trace, launch_pool, launch_nee and the launch tables above them):
the launchers pick one of some hundred template instantiations by the scene, the frame's modes and what is bound, and a
wrong pick can still render the right frame (the full kernel where the lean one would do costs 3.5 %).  The reported name is the only
place where that shows, so every family's picks are pinned here, byte for byte, on 16 x 16 frames of 1 spp and 2 bounces."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import fuzz_parity as fz  # noqa: E402
from gpupathtracer_amd import lib, scenes  # noqa: E402
from gpupathtracer_amd import types as T  # noqa: E402

pytestmark = pytest.mark.gpu

W, H = 16, 16
INSIDE = dict(position=(0.0, 0.0, 2.4), yaw=-90.0, pitch=0.0)
MIRROR_FLOOR, MIRROR_CUBE = 3, 1  # geometry indices in scenes.cornell_mirror_scene
POOL_SWITCHES = ("FF_POOL", "FF_POOL_QUORUM", "FF_POOL_SLICE", "FF_POOL_REFILL", "FF_POOL_LEAVE", "FF_POOL_BATCH_MIN", "FF_POOL_STACK_LEVELS")


def _render(t, **params):
    t.render(scenes.posed_camera(W, H, **INSIDE), lib.render_params(W, H, 2, 1, seed=3, **params))
    return t.kernel_name()


@pytest.fixture
def own(monkeypatch):
    """A tracer of this test's own, created under the default switches."""
    for k in POOL_SWITCHES + ("FF_NO_START_RECORDS", "FF_REUSE_MIN_SPP", "FF_BLOCK_THREADS"):
        monkeypatch.delenv(k, raising=False)
    with lib.Tracer(0) as t:
        yield t


# ---- the trace family ----------------------------------------------------------------------------------------------------------------

TRACE = [  # scene, statistics, trace mode, expected name
    ("wahoo", False, T.TRACE_BVH, "trace_bvh_kernel<false, 1024, false, 0, false>"),
    ("wahoo", True, T.TRACE_BVH, "trace_bvh_kernel<true, 1024, false, 0, false>"),
    ("mirror", False, T.TRACE_BVH, "trace_bvh_kernel<false, 1024, true, 0, false>"),
    ("mirror", True, T.TRACE_BVH, "trace_bvh_kernel<true, 1024, true, 0, false>"),
    ("wahoo", False, T.TRACE_BRUTE_FORCE, "trace_brute_kernel<false>"),
    ("wahoo", True, T.TRACE_BRUTE_FORCE, "trace_brute_kernel<true>"),
    ("mirror", False, T.TRACE_BRUTE_FORCE, "trace_brute_kernel<false>"),
]


def _scene(name):
    return scenes.cornell_wahoo_scene() if name == "wahoo" else scenes.cornell_mirror_scene()


def test_trace_kernel_names(own):
    """One-off 1-spp frames trace their primary rays themselves: the lane-owned kernel without and with the extras, with and without
    statistics, and the brute-force kernel."""
    for name, stats, trace, want in TRACE:
        own.upload_scene(_scene(name))
        own.set_collect_stats(stats)
        assert _render(own, trace_mode=trace) == want, (name, stats, trace)
    own.set_collect_stats(False)


START = [  # scene, statistics, expected name: only the diffuse scene starts from records
    ("wahoo", False, "trace_bvh_kernel<false, 1024, false, 0, false, true>"),
    ("wahoo", True, "trace_bvh_kernel<true, 1024, false, 0, false, true>"),
    ("mirror", False, "trace_bvh_kernel<false, 1024, true, 0, false>"),
]


def test_start_record_kernel_names(monkeypatch):
    """Every frame on stored hits (FF_REUSE_MIN_SPP=1, as tests/test_gpu_start_records.py arranges it): the diffuse scene runs the
    START instantiation, named by six parameters; a scene with extras keeps the raw-hit kernel and its five."""
    for k in POOL_SWITCHES + ("FF_NO_START_RECORDS", "FF_BLOCK_THREADS"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("FF_REUSE_MIN_SPP", "1")
    with lib.Tracer(0) as t:
        for name, stats, want in START:
            t.upload_scene(_scene(name))
            t.set_collect_stats(stats)
            assert _render(t) == want, (name, stats)


POOL = [
    ("wahoo", False, "trace_pool_kernel<false, 1024, false>"),
    ("wahoo", True, "trace_pool_kernel<true, 1024, false>"),
    ("mirror", False, "trace_pool_kernel<false, 1024, true>"),
    ("mirror", True, "trace_pool_kernel<true, 1024, true>"),
]


def test_pool_kernel_names(monkeypatch):
    """FF_POOL=1: the job-pool kernel, in BVH mode only."""
    for k in POOL_SWITCHES + ("FF_NO_START_RECORDS", "FF_REUSE_MIN_SPP", "FF_BLOCK_THREADS"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("FF_POOL", "1")
    with lib.Tracer(0) as t:
        for name, stats, want in POOL:
            t.upload_scene(_scene(name))
            t.set_collect_stats(stats)
            assert _render(t) == want, (name, stats)
        t.set_collect_stats(False)
        assert _render(t, trace_mode=T.TRACE_BRUTE_FORCE) == "trace_brute_kernel<false>"


BIG = [  # crowd of tools/fuzz_parity.py rand_scene (as tests/test_gpu_fuzz.py renders it), statistics, expected name
    (80, False, "trace_bvh_kernel<false, 1024, true, 1, false>"),
    (80, True, "trace_bvh_kernel<true, 1024, true, 1, false>"),
    (500, False, "trace_bvh_kernel<false, 1024, true, 2, false>"),
    (500, True, "trace_bvh_kernel<true, 1024, true, 2, false>"),
]


def test_big_scene_trace_kernel_names(own):
    """33-128 geometries: the tree over the geometries with the records in LDS; more: the records in global memory."""
    for crowd, stats, want in BIG:
        scene = fz.rand_scene(np.random.default_rng(3), small=True, crowd=crowd)
        assert (32 < len(scene) <= 128) if crowd == 80 else len(scene) > 128
        own.upload_scene(scene)
        own.set_collect_stats(stats)
        assert _render(own) == want, (crowd, stats)
    own.set_collect_stats(False)


# ---- the NEE family ------------------------------------------------------------------------------------------------------------------

NEE = {  # (ENV, TEX, GLOSSY, CAM) -> the name's tail after "nee_path_kernel<MODE, BIG": the parameters up to the last one that is 1
    (0, 0, 0, 0): "nee_path_kernel<1, 0>",
    (1, 0, 0, 0): "nee_path_kernel<1, 0, 1>",
    (0, 1, 0, 0): "nee_path_kernel<1, 0, 0, 1>",
    (1, 1, 0, 0): "nee_path_kernel<1, 0, 1, 1>",
    (0, 0, 1, 0): "nee_path_kernel<1, 0, 0, 0, 1>",
    (1, 0, 1, 0): "nee_path_kernel<1, 0, 1, 0, 1>",
    (0, 1, 1, 0): "nee_path_kernel<1, 0, 0, 1, 1>",
    (1, 1, 1, 0): "nee_path_kernel<1, 0, 1, 1, 1>",
    (0, 0, 0, 1): "nee_path_kernel<1, 0, 0, 0, 0, 1>",
    (1, 0, 0, 1): "nee_path_kernel<1, 0, 1, 0, 0, 1>",
    (0, 1, 0, 1): "nee_path_kernel<1, 0, 0, 1, 0, 1>",
    (1, 1, 0, 1): "nee_path_kernel<1, 0, 1, 1, 0, 1>",
    (0, 0, 1, 1): "nee_path_kernel<1, 0, 0, 0, 1, 1>",
    (1, 0, 1, 1): "nee_path_kernel<1, 0, 1, 0, 1, 1>",
    (0, 1, 1, 1): "nee_path_kernel<1, 0, 0, 1, 1, 1>",
    (1, 1, 1, 1): "nee_path_kernel<1, 0, 1, 1, 1, 1>",
}
NEE_BRUTE = {(0, 0, 0, 0): "nee_path_kernel<0, 0>", (1, 1, 1, 1): "nee_path_kernel<0, 0, 1, 1, 1, 1>"}


def test_nee_kernel_names(own):
    """The sixteen combinations of an environment, a bound albedo texture, a rough mirror and per-sample camera rays on the mirror
    scene in BVH mode, and the two corners in brute-force mode."""
    texture = own.create_texture(np.full((4, 4, 3), 0.5, np.float32))
    sky = np.full((4, 8, 3), 0.3, np.float32)
    try:
        for (env, tex, glossy, cam), want in NEE.items():
            own.upload_scene(scenes.cornell_mirror_scene())  # (an upload drops the bindings of the scene before it)
            if env:
                own.set_environment(sky, 1.0, 0.0)
            else:
                own.clear_environment()
            if tex:
                own.set_albedo_texture(MIRROR_FLOOR, texture)
            if glossy:
                own.set_roughness(MIRROR_CUBE, 0.3)
            own.set_camera_sampling(lib.camera_sampling(T.PIXEL_BOX, 0.08, 2.5) if cam else None)
            assert _render(own, shade_mode=T.SHADE_DIFFUSE_PATH_NEE) == want, (env, tex, glossy, cam)
            if (env, tex, glossy, cam) in NEE_BRUTE:
                got = _render(own, shade_mode=T.SHADE_DIFFUSE_PATH_NEE, trace_mode=T.TRACE_BRUTE_FORCE)
                assert got == NEE_BRUTE[(env, tex, glossy, cam)], (env, tex, glossy, cam)
    finally:
        own.set_camera_sampling(None)
        own.clear_environment()
        own.destroy_texture(texture)
