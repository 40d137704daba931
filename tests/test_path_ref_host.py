"""The float64 path walker (tests/path_ref.py) on the host: against the CPU oracle's FF_SHADE_DIFFUSE_PATH frames at depth - the random
number counters, the glass definition, the throughput and the accumulation order - with the oracle's own intersector, within the
walker's excuse cap; and the walker's two modes against each other (the project's z-test on block means, and equality with an empty
light table).  Needs no GPU."""
import numpy as np
import pytest

from gpupathtracer_amd import lib, scenes
from gpupathtracer_amd import types as T
import nee_ref
import path_ref
from oracle_lib import oracle_intersect, oracle_render

NEE, PATH = T.SHADE_DIFFUSE_PATH_NEE, T.SHADE_DIFFUSE_PATH
W, H = 24, 16
POSE = dict(position=(0.0, 0.0, 2.4), yaw=-90.0, pitch=10.0)  # test_gpu_nee.py's INSIDE pose, tilted up until the ceiling light is in view
EXCUSE_CAP = 0.10

SCENES = {
    "C2_cube": lambda: scenes.cornell_wahoo_scene(wahoo=scenes.load_mesh("cube")),  # (the cube for wahoo: the oracle's loop is brute force)
    "mirror": scenes.cornell_mirror_scene,
    "glass": scenes.cornell_glass_scene,
    "spheres": scenes.cornell_spheres_scene,
}


def intersector(scene):
    return lambda o, d: oracle_intersect(scene, o, d)


@pytest.fixture(scope="module")
def built():
    return {name: make() for name, make in SCENES.items()}


@pytest.mark.parametrize("name", sorted(SCENES))
@pytest.mark.parametrize("spp", [1, 3])
@pytest.mark.parametrize("bounces", [1, 2, 3, 5])
def test_walker_matches_the_oracle(built, name, spp, bounces):
    scene = built[name]
    c = scenes.posed_camera(W, H, **POSE)
    p = lib.render_params(W, H, bounces, spp, seed=(5 << 32) | 41, shade_mode=PATH)
    ref = oracle_render(scene, c, p, threads=4)[1].astype(np.float64)
    got, excused, stats = path_ref.walk(intersector(scene), scene, c, p)
    hit = stats["hit"]
    dev = np.abs(got - ref) / (path_ref.RTOL * np.abs(ref) + path_ref.ATOL)  # in units of the rule's allowance
    judged = hit & ~excused
    worst = dev[judged].max() if judged.any() else 0.0
    print(f"{name} bounces {bounces} spp {spp}: largest deviation {worst:.4f} of the allowance (absolute {np.abs(got - ref)[judged].max():.3g}), "
          f"excused {excused[hit].mean():.4f} of {hit.sum()} hit pixels, {stats['refracted_segments']} refracted segments")
    assert hit.sum() > 0.9 * W * H and ref[hit].max() > 0.0
    assert np.all(got[~hit] == 0.0) and np.all(ref[~hit] == 0.0)
    assert excused[hit].mean() <= EXCUSE_CAP
    assert 4.0 * worst <= 1.0, "the bounces = 2 rule no longer holds with the margin path_ref.py's docstring states"
    if name == "glass" and bounces >= 3:
        assert stats["refracted_segments"] > 0
    if name in ("mirror", "glass", "spheres") and bounces == 5 and spp == 3:
        assert stats["emitter_hits_after_specular"] > 0


@pytest.mark.parametrize("bounces", [3, 4])
def test_nee_and_path_mode_of_the_walker_agree_in_expectation(bounces):
    """test_gpu_nee.py's z-test on 8x8 block means, applied to the reference itself."""
    scene = nee_ref.triangle_light_scene()
    c = scenes.posed_camera(W, H, **POSE)
    seeds = 8
    imgs = {}
    for mode in (PATH, NEE):
        imgs[mode] = np.stack([path_ref.walk(intersector(scene), scene, c, lib.render_params(W, H, bounces, 1, seed=1000 + s, shade_mode=mode))[0]
                               for s in range(seeds)])
    assert imgs[PATH].mean() > 0.0

    def blocks(x):
        return x.reshape(seeds, H // 8, 8, W // 8, 8, 3).mean(axis=(2, 4))

    a, b = blocks(imgs[PATH]), blocks(imgs[NEE])
    se = np.sqrt(a.var(0, ddof=1) / seeds + b.var(0, ddof=1) / seeds) + 1e-7
    z = np.abs(a.mean(0) - b.mean(0)) / se
    print(f"bounces {bounces}: block means off by at most {z.max():.2f} standard errors")
    assert z.max() < 5.0, f"block mean off by {z.max():.2f} standard errors"


@pytest.mark.parametrize("bounces", [3, 4])
def test_empty_light_table_makes_the_modes_equal(bounces):
    scene = nee_ref.sphere_light_scene()
    assert len(lib.light_table(scene)[0]["area"]) == 0
    w, h = W, H
    c = scenes.posed_camera(w, h, **POSE)
    out = {}
    for mode in (PATH, NEE):
        out[mode] = path_ref.walk(intersector(scene), scene, c, lib.render_params(w, h, bounces, 1, seed=3, shade_mode=mode))
    assert out[PATH][0].max() > 0.0
    assert np.all(np.abs(out[PATH][0] - out[NEE][0]) <= 1e-12)
    assert np.array_equal(out[PATH][1], out[NEE][1])
