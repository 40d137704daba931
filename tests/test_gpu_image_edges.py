"""ff_gbuffer, ff_denoise, ff_denoise_temporal and ff_taa on the GPU at the edges the 160x90 comparisons do not reach: image
sizes that leave partial 16x16 workgroups, 8x8 tiles and 64x4 row blocks (and images narrower than all of them), the shipped
1920x1080, parameters far from the defaults, changes of size between calls, exact power-of-two scaling, and non-finite
radiance (ff_api.h's rule: it stays in its own pixel and never enters the history).  Each filter is compared with its float64
reference (tests/gbuffer_ref.py, temporal_ref.py, taa_ref.py) under the tolerances and near-threshold excuses of
test_gpu_denoise.py, test_gpu_temporal.py and test_gpu_taa.py."""
import numpy as np
import pytest

from gpupathtracer_amd import lib, scenes
from gpupathtracer_amd import types as T
from gbuffer_ref import denoise_ref, filterable, oracle_gbuffer
from taa_ref import TaaRef
from temporal_ref import TemporalRef, scene_models

pytestmark = pytest.mark.gpu

# (width, height): 1-pixel rows and columns, smaller than a 16x16 workgroup, an 8x8 tile or a 64x4 row block, and one
# partial block past each
SIZES = [(1, 1), (1, 37), (37, 1), (2, 3), (7, 5), (15, 17), (17, 15), (63, 4), (65, 5), (161, 91), (257, 33)]
HD = (1920, 1080)
PARAM_SIZES = [(161, 91), (15, 17)]
SHARE_MIN_PIXELS = 1000  # the share bounds of the 160x90 tests apply from this many filterable pixels on (one pixel of a 1x37 image is 3 %)
# as test_gpu_temporal.py: three poses a few pixels apart at 160x90
POSES = [((0.0, 0.0, 2.4), -90.0), ((0.06, -0.04, 2.4), -89.3), ((0.1, -0.02, 2.37), -88.8)]
SCENES = ["cornell_wahoo_scene", "cornell_spheres_scene"]
DENOISE_FLAGS = [0, T.DENOISE_SAME_GEOMETRY, T.DENOISE_SAME_GEOMETRY | T.DENOISE_DEMODULATE_ALBEDO]
TAA_FLAGS = [0, T.TAA_BILINEAR, T.TAA_NO_CLAMP, T.TAA_BILINEAR | T.TAA_NO_CLAMP]


def cam(pose, w, h):
    (x, y, z), yaw = POSES[pose]
    return scenes.posed_camera(w, h, position=(x, y, z), yaw=yaw, pitch=0.0)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def size_id(s):
    return f"{s[0]}x{s[1]}"


def synthetic_radiance(seed, w, h):
    """test_gpu_temporal's seeded radiance: a smooth image times noise, a few pixels far brighter than their neighbours (every
    channel in [0.03, 10])."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    smooth = np.stack([0.4 + 0.3 * np.sin(xx / 17.0), 0.3 + 0.2 * np.cos(yy / 11.0), 0.2 + 0.001 * xx], -1)
    rad = smooth * rng.uniform(0.3, 1.7, size=(h, w, 3)) * np.where(rng.random((h, w, 1)) < 0.02, 8.0, 1.0)
    return rad.astype(np.float32)


_SCENES = {}


def scene_of(name):
    if name not in _SCENES:
        _SCENES[name] = getattr(scenes, name)()
    return _SCENES[name]


def jitter_of(i):
    return lib.jitter_sequence(i, 16)


@pytest.fixture(scope="module")
def guides():
    """guides(scene, pose, w, h, jitter=(0, 0)): ff_gbuffer of the scene at that pose, size and jitter, from a Tracer of the
    module's own (the tracer under test keeps its state); images up to 257x33 are cached."""
    tracers, cache = {}, {}

    def get(scene_name, pose, w, h, jitter=(0.0, 0.0)):
        key = (scene_name, pose, w, h, tuple(jitter))
        if key in cache:
            return cache[key]
        if scene_name not in tracers:
            tracers[scene_name] = lib.Tracer(0)
            tracers[scene_name].upload_scene(scene_of(scene_name))
        t = tracers[scene_name]
        t.set_pixel_jitter(*jitter)
        try:
            gb = t.gbuffer(cam(pose, w, h), lib.render_params(w, h))
        finally:
            t.set_pixel_jitter(0.0, 0.0)
        if w * h <= 257 * 33:
            cache[key] = gb
        return gb

    yield get
    for t in tracers.values():
        t.close()


# ---- ff_gbuffer ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("size", SIZES, ids=size_id)
@pytest.mark.parametrize("scene_name,grid", [("cornell_wahoo_scene", T.GRID_FULL), ("cornell_wahoo_scene", T.GRID_REFERENCE_FLOOR),
                                             ("cornell_spheres_scene", T.GRID_FULL)])
def test_gbuffer_matches_the_oracle_at_odd_sizes(tracer, scene_name, grid, size):
    w, h = size
    scene, c, params = scene_of(scene_name), cam(0, w, h), lib.render_params(w, h, grid_mode=grid)
    tracer.upload_scene(scene)
    got, want = tracer.gbuffer(c, params), oracle_gbuffer(scene, c, params)
    for k in want:
        assert got[k].shape == want[k].shape, k
        bad = np.argwhere(bits(got[k]) != bits(want[k]))
        assert bad.size == 0, f"{k}: {len(bad)} values differ, first at {bad[:3].tolist()}"
    if grid == T.GRID_REFERENCE_FLOOR:
        assert (got["ids"][(h // 16) * 16:, :] == -1).all() and (got["ids"][:, (w // 16) * 16:] == -1).all()
        if w < 16 or h < 16:
            assert (got["ids"] == -1).all() and not got["depth"].any() and not got["position"].any()
    if w * h >= 100 and (grid == T.GRID_FULL or (w >= 16 and h >= 16)):
        assert (got["ids"][..., 0] >= 0).any()


# ---- ff_denoise ---------------------------------------------------------------------------------------------------------

def check_denoise(tracer, gb, dn, seed=2024):
    """ff_denoise against denoise_ref on test_gpu_denoise's radiance; returns the largest relative error."""
    h, w = gb["ids"].shape[:2]
    rad = synthetic_radiance(seed, w, h)
    _, out = tracer.denoise(rad, gb, dn)
    ref = denoise_ref(rad, gb, dn.iterations, dn.sigma_color, dn.sigma_normal, dn.sigma_plane, dn.flags)
    big = np.abs(ref) > 1e-3
    err = float((np.abs(out.astype(np.float64) - ref)[big] / np.abs(ref)[big]).max(initial=0.0))
    print(f"ff_denoise {w}x{h} iterations {dn.iterations} sigmas {dn.sigma_color:g} {dn.sigma_normal:g} {dn.sigma_plane:g} "
          f"flags {dn.flags}: max rel err {err:.3g}")
    assert err <= 1e-4, err
    keep = ~filterable(gb["ids"])
    assert np.array_equal(bits(out[keep]), bits(rad[keep]))
    return err


@pytest.mark.parametrize("flags", DENOISE_FLAGS)
@pytest.mark.parametrize("scene_name", SCENES)
@pytest.mark.parametrize("size", SIZES, ids=size_id)
def test_denoise_matches_the_reference_at_odd_sizes(tracer, guides, size, scene_name, flags):
    check_denoise(tracer, guides(scene_name, 0, *size), lib.denoise_params(flags=flags))


def test_denoise_matches_the_reference_at_1080p(tracer, guides):
    check_denoise(tracer, guides("cornell_wahoo_scene", 0, *HD), lib.denoise_params())


DENOISE_PARAMS = {f"iterations_{n}": dict(iterations=n) for n in (1, 2, 7, 10)}
for _name, _default in (("sigma_color", 4.0), ("sigma_normal", 0.1), ("sigma_plane", 0.1)):
    for _f in (0.125, 8.0):
        DENOISE_PARAMS[f"{_name}_x{_f:g}"] = {_name: _default * _f}


@pytest.mark.parametrize("case", sorted(DENOISE_PARAMS))
@pytest.mark.parametrize("size", PARAM_SIZES, ids=size_id)
def test_denoise_parameters_match_the_reference(tracer, guides, size, case):
    check_denoise(tracer, guides("cornell_wahoo_scene", 0, *size), lib.denoise_params(**DENOISE_PARAMS[case]))


# ---- ff_denoise_temporal ----------------------------------------------------------------------------------------------

# test_gpu_temporal.MODES: (parameters, poses, share of the filterable pixels that must be checked)
MODES = {
    "moving_accumulation": (dict(iterations=0, feedback_pass=-1), (0, 1, 2), 0.98),
    "moving_one_pass": (dict(iterations=1, feedback_pass=0), (0, 1, 2), 0.5),
    "at_rest_five_passes": ({}, (0, 0, 0, 0, 0), 1.0),
}


def check_temporal(tracer, guides, scene_name, w, h, tp, poses, min_checked, max_near=0.005):
    """One ff_denoise_temporal sequence against TemporalRef under test_gpu_temporal's rules; returns (max rel err, excused share).
    A moving sequence's tolerance grows with the image past 160 pixels: the float32 error of the reprojected pixel coordinate
    (and so of the bilinear weights) is relative to the coordinate."""
    tol = 1e-4 * (max(1.0, w / 160.0) if len(set(poses)) > 1 else 1.0)
    tracer.upload_scene(scene_of(scene_name))
    tracer.temporal_reset()
    ref, models = TemporalRef(), scene_models(scene_of(scene_name))
    worst, excused_share = 0.0, 0.0
    for i, k in enumerate(poses):
        gb, c = guides(scene_name, k, w, h), cam(k, w, h)
        rad = synthetic_radiance(100 + i, w, h)
        _, out = tracer.denoise_temporal(rad, gb, c, tp)
        _, length = tracer.temporal_history()
        r = ref.step(rad, gb, c, models, tp)
        near, excused = r["near"], r["tainted"]
        f = filterable(gb["ids"])
        big = np.abs(r["out"]) > 1e-3
        err = np.where(big, np.abs(out.astype(np.float64) - r["out"]) / np.where(big, np.abs(r["out"]), 1.0), 0.0).max(-1)
        e = float(err[~excused].max(initial=0.0))
        worst = max(worst, e)
        if f.any():
            excused_share = max(excused_share, float((excused & f).sum() / f.sum()))
        if f.sum() >= SHARE_MIN_PIXELS:
            assert near.mean() < max_near, near.mean()
            assert (f & ~excused).sum() >= min_checked * f.sum(), (excused & f).sum()
        assert e <= tol, (i, e, np.argwhere((err > tol) & ~excused)[:5])
        whole = ~excused & (r["length"] == np.round(r["length"]))
        assert np.array_equal(length[whole], r["length"][whole])
        assert np.allclose(length[~excused], r["length"][~excused], rtol=1e-5, atol=0)
    print(f"ff_denoise_temporal {scene_name} {w}x{h} poses {poses}: max rel err {worst:.3g}, excused share {excused_share:.4f}")
    return worst, excused_share


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("scene_name", SCENES)
@pytest.mark.parametrize("size", SIZES, ids=size_id)
def test_temporal_matches_the_reference_at_odd_sizes(tracer, guides, size, scene_name, mode):
    over, poses, min_checked = MODES[mode]
    check_temporal(tracer, guides, scene_name, *size, lib.temporal_params(**over), poses, min_checked)


def test_temporal_matches_the_reference_at_1080p(tracer, guides):
    # At rest, two calls (the float64 passes take most of a minute a call at this size).  A moving camera at 1080p puts ~3 % of
    # the pixels within the reference's near-threshold band (1e-5 of a coordinate of ~1000 pixels), past the 0.5 % the 160x90
    # comparisons allow: the moving paths are compared at every size up to 257x33 instead.
    over, poses, min_checked = MODES["at_rest_five_passes"]
    check_temporal(tracer, guides, "cornell_wahoo_scene", *HD, lib.temporal_params(**over), poses[:2], min_checked)


MOVING, AT_REST = (0, 1, 2), (0, 0, 0, 0)
ACCUMULATE = dict(iterations=0, feedback_pass=-1)
# name -> (parameters, poses, checked share, near share).  Several passes are compared at rest, as MODES does.  reuse_normal 1
# and reuse_plane 0 put every tap of a flat surface on its threshold: the reference excuses those pixels, and what is left is checked.
TEMPORAL_PARAMS = {
    "iterations_0": (ACCUMULATE, MOVING, 0.98, 0.005),
    "iterations_10": (dict(iterations=10), AT_REST, 1.0, 0.005),
    **{f"iterations_3_feedback_{fp}": (dict(iterations=3, feedback_pass=fp), AT_REST, 1.0, 0.005) for fp in (-1, 0, 1, 2)},
    "max_history_1": (dict(ACCUMULATE, max_history=1), MOVING, 0.98, 0.005),
    "max_history_2": (dict(ACCUMULATE, max_history=2), MOVING, 0.98, 0.005),
    "max_history_2_at_rest": (dict(max_history=2), AT_REST, 1.0, 0.005),
    "variance_history_1": (dict(iterations=1, feedback_pass=0, variance_history=1), MOVING, 0.5, 0.005),
    "variance_history_20": (dict(iterations=1, feedback_pass=0, variance_history=20), MOVING, 0.5, 0.005),
    "reuse_normal_-1": (dict(ACCUMULATE, reuse_normal=-1.0), MOVING, 0.98, 0.005),
    "reuse_normal_1": (dict(ACCUMULATE, reuse_normal=1.0), MOVING, 0.0, 1.0),
    "reuse_plane_0": (dict(ACCUMULATE, reuse_plane=0.0), MOVING, 0.0, 1.0),
}


@pytest.mark.parametrize("case", sorted(TEMPORAL_PARAMS))
@pytest.mark.parametrize("size", PARAM_SIZES, ids=size_id)
def test_temporal_parameters_match_the_reference(tracer, guides, size, case):
    over, poses, min_checked, max_near = TEMPORAL_PARAMS[case]
    check_temporal(tracer, guides, "cornell_wahoo_scene", *size, lib.temporal_params(**over), poses, min_checked, max_near)


# ---- ff_taa -------------------------------------------------------------------------------------------------------------

TAA_SEQUENCES = {"at_rest": (0, 0, 0), "sliding": (0, 1, 2)}


def check_taa(tracer, guides, w, h, p, seq, scene_name="cornell_wahoo_scene"):
    """One ff_taa sequence against TaaRef under test_gpu_taa's rules; returns (max rel err, excused share).  Sliding, the motion
    and output tolerances grow with the image past 160 pixels: the float32 error of a pixel coordinate is relative to it, and
    the resampled history moves with it."""
    tracer.upload_scene(scene_of(scene_name))
    tracer.taa_reset()
    ref, models = TaaRef(), scene_models(scene_of(scene_name))
    worst, excused_share = 0.0, 0.0
    grow = max(1.0, w / 160.0) if seq != "at_rest" else 1.0
    tol, motion_tol = 1e-3 * grow, 2e-3 * grow
    for i, k in enumerate(TAA_SEQUENCES[seq]):
        gb, c = guides(scene_name, k, w, h, jitter_of(i)), cam(k, w, h)
        rad = synthetic_radiance(100 + i, w, h)
        _, out = tracer.taa(rad, gb, c, p)
        motion, length = tracer.taa_history()
        r = ref.step(rad, gb, c, models, p)
        excused = r["tainted"]
        err = (np.abs(out.astype(np.float64) - r["out"]) / np.maximum(np.abs(r["out"]), 0.1)).max(-1)
        merr = float(np.abs(motion - r["motion"]).max(-1)[~excused].max(initial=0.0))
        e = float(err[~excused].max(initial=0.0))
        worst, excused_share = max(worst, e), max(excused_share, float(excused.mean()))
        if seq == "at_rest":
            assert not excused.any() and not motion.any()
        elif w * h >= SHARE_MIN_PIXELS:
            assert excused.mean() <= 0.1, excused.mean()
        assert e <= tol, (i, e, np.argwhere((err > tol) & ~excused)[:5])
        assert merr <= motion_tol, (i, merr)
        assert np.array_equal(length[~excused], r["length"][~excused].astype(np.float32))
    if seq == "at_rest":
        assert (r["length"] == 3).all()
    print(f"ff_taa {w}x{h} {seq} flags {p.flags} alpha_min {p.alpha_min:g} gamma {p.gamma:g}: max rel err {worst:.3g}, "
          f"excused share {excused_share:.4f}")
    return worst, excused_share


@pytest.mark.parametrize("seq", sorted(TAA_SEQUENCES))
@pytest.mark.parametrize("flags", TAA_FLAGS)
@pytest.mark.parametrize("size", SIZES, ids=size_id)
def test_taa_matches_the_reference_at_odd_sizes(tracer, guides, size, flags, seq):
    check_taa(tracer, guides, *size, lib.taa_params(flags=flags, alpha_min=0.2, gamma=1.25), seq)


def test_taa_matches_the_reference_at_1080p(tracer, guides):
    # At rest (nothing excused).  Sliding at 1080p, the reference's near-threshold band (1e-5 of a coordinate of ~1000 pixels)
    # and the 16 Catmull-Rom taps that spread it excuse ~18 % of the pixels, past the 10 % the 160x90 comparisons allow.
    check_taa(tracer, guides, *HD, lib.taa_params(alpha_min=0.2, gamma=1.25), "at_rest")


TAA_PARAMS = {"alpha_min_1": dict(alpha_min=1.0), "alpha_min_0.01": dict(alpha_min=0.01), "gamma_0.05": dict(gamma=0.05),
              "gamma_100": dict(gamma=100.0)}


@pytest.mark.parametrize("seq", sorted(TAA_SEQUENCES))
@pytest.mark.parametrize("case", sorted(TAA_PARAMS))
@pytest.mark.parametrize("size", PARAM_SIZES, ids=size_id)
def test_taa_parameters_match_the_reference(tracer, guides, size, case, seq):
    check_taa(tracer, guides, *size, lib.taa_params(**TAA_PARAMS[case]), seq)


# ---- a change of size drops the history -----------------------------------------------------------------------------------

def _first_call(kind, w, h, gb, rad, c):
    """What a fresh Tracer's first call returns: (rgb8, radiance, motion, length)."""
    with lib.Tracer(0) as fresh:
        fresh.upload_scene(scene_of("cornell_wahoo_scene"))
        if kind == "temporal":
            return (*fresh.denoise_temporal(rad, gb, c), *fresh.temporal_history())
        return (*fresh.taa(rad, gb, c), *fresh.taa_history())


@pytest.mark.parametrize("kind", ["temporal", "taa"])
@pytest.mark.parametrize("other", [(90, 160), HD], ids=size_id)
def test_a_change_of_size_starts_afresh(tracer, guides, kind, other):
    """160x90 -> other -> 160x90, two calls at each size: the first call after each change equals a fresh Tracer's first call bit
    for bit and reports length 1 on every pixel that keeps a history."""
    tracer.upload_scene(scene_of("cornell_wahoo_scene"))
    tracer.temporal_reset()
    tracer.taa_reset()
    fresh = {}
    n = 0
    for stage, (w, h) in enumerate([(160, 90), other, (160, 90)]):
        for j, k in enumerate((1, 2)):
            jit = jitter_of(n) if kind == "taa" else (0.0, 0.0)
            gb, c, rad = guides("cornell_wahoo_scene", k, w, h, jit), cam(k, w, h), synthetic_radiance(200 + n, w, h)
            n += 1
            if kind == "temporal":
                got = (*tracer.denoise_temporal(rad, gb, c), *tracer.temporal_history())
            else:
                got = (*tracer.taa(rad, gb, c), *tracer.taa_history())
            if stage == 0 or j == 1:
                assert got[3].max() == (j + 1), (stage, j)  # (the history continues within a size)
                continue
            key = (w, h, k, jit)
            if key not in fresh:
                fresh[key] = _first_call(kind, w, h, gb, rad, c)
            want = fresh[key]
            assert np.array_equal(got[0], want[0]) and all(np.array_equal(bits(a), bits(b)) for a, b in zip(got[1:], want[1:])), (w, h)
            keeps = filterable(gb["ids"]) if kind == "temporal" else np.ones((h, w), bool)
            assert (got[3][keeps] == 1).all() and not got[3][~keeps].any() and not got[2].any()


# ---- power-of-two scaling is exact --------------------------------------------------------------------------------------

@pytest.mark.parametrize("scale", [2.0 ** -20, 2.0 ** 20], ids=["2^-20", "2^20"])
def test_power_of_two_scaling_is_exact(tracer, guides, scale):
    """The radiance keeps every channel in [0.03, 10], so no value any kernel computes from it is subnormal or overflows at
    either scale: every output is exactly the scaled output."""
    s = np.float32(scale)
    w, h = 161, 91
    scene_name = "cornell_wahoo_scene"
    tracer.upload_scene(scene_of(scene_name))
    gb = guides(scene_name, 0, w, h)
    rad = synthetic_radiance(2024, w, h)
    for flags in DENOISE_FLAGS:
        _, a = tracer.denoise(rad, gb, lib.denoise_params(flags=flags))
        _, b = tracer.denoise(rad * s, gb, lib.denoise_params(flags=flags))
        assert np.array_equal(bits(b), bits(a * s)), ("ff_denoise", flags)

    def sequences(run, reset, history, params, poses, jitter):
        outs = []
        for k in (1.0, s):
            reset()
            seq = []
            for i, pose in enumerate(poses):
                g = guides(scene_name, pose, w, h, jitter(i))
                _, o = run(synthetic_radiance(100 + i, w, h) * np.float32(k), g, cam(pose, w, h), params)
                seq.append((o, *history()))
            outs.append(seq)
        for i, ((o1, m1, l1), (o2, m2, l2)) in enumerate(zip(*outs)):
            assert np.array_equal(bits(o2), bits(o1 * s)), i
            assert np.array_equal(bits(m1), bits(m2)) and np.array_equal(bits(l1), bits(l2)), i

    for over in ({}, MODES["moving_one_pass"][0], MODES["moving_accumulation"][0]):
        for poses in ((0, 1, 2), (0, 0, 0)):
            sequences(tracer.denoise_temporal, tracer.temporal_reset, tracer.temporal_history, lib.temporal_params(**over), poses,
                      lambda i: (0.0, 0.0))
    for flags in TAA_FLAGS:
        for poses in ((0, 1, 2), (0, 0, 0)):
            sequences(tracer.taa, tracer.taa_reset, tracer.taa_history, lib.taa_params(flags=flags), poses, jitter_of)


# ---- non-finite radiance ------------------------------------------------------------------------------------------------

W, H = 160, 90


def poisoned_pixels(gb):
    """(NaN pixel, +Inf pixel): two filterable pixels away from the borders and from each other."""
    f = filterable(gb["ids"])
    f[:4], f[-4:], f[:, :4], f[:, -4:] = False, False, False, False
    cand = np.argwhere(f)
    return tuple(cand[len(cand) // 3]), tuple(cand[(2 * len(cand)) // 3])


def poison(rad, a, b):
    rad = rad.copy()
    rad[a] = np.nan
    rad[b] = np.inf
    return rad


def test_denoise_keeps_a_non_finite_pixel_to_itself(tracer, guides):
    gb = guides("cornell_wahoo_scene", 0, W, H)
    a, b = poisoned_pixels(gb)
    rad = poison(synthetic_radiance(5, W, H), a, b)
    missed = {k: v.copy() for k, v in gb.items()}
    missed["ids"][a] = missed["ids"][b] = -1
    others = np.ones((H, W), bool)
    others[a] = others[b] = False
    for flags in DENOISE_FLAGS:
        _, out = tracer.denoise(rad, gb, lib.denoise_params(flags=flags))
        _, ref = tracer.denoise(rad, missed, lib.denoise_params(flags=flags))
        assert np.isfinite(out[others]).all(), flags
        assert np.array_equal(bits(out[others]), bits(ref[others])), flags


def _poisoned_sequence(tracer, guides, kind, seq, p):
    """Three 1-spp frames (8 bounces) at the sequence's poses, the second with one NaN and one +Inf pixel; checks ff_api.h's rule."""
    scene_name = "cornell_wahoo_scene"
    tracer.upload_scene(scene_of(scene_name))
    tracer.temporal_reset()
    tracer.taa_reset()
    poses = TAA_SEQUENCES[seq]
    a = b = None
    try:
        for i, k in enumerate(poses):
            jit = jitter_of(i) if kind == "taa" else (0.0, 0.0)
            gb, c = guides(scene_name, k, W, H, jit), cam(k, W, H)
            tracer.set_pixel_jitter(*jit)
            _, rad = tracer.render(c, lib.render_params(W, H, 8, 1, 500 + i))
            if i == 1:
                a, b = poisoned_pixels(gb)
                rad = poison(rad, a, b)
            if kind == "temporal":
                _, out = tracer.denoise_temporal(rad, gb, c, p)
                _, length = tracer.temporal_history()
            else:
                _, out = tracer.taa(rad, gb, c, p)
                _, length = tracer.taa_history()
            finite = np.isfinite(out).all(-1)
            if i == 1:
                finite[a] = finite[b] = True  # (its own pixel may be non-finite in that call)
            assert finite.all(), (i, np.argwhere(~finite)[:5].tolist())
    finally:
        tracer.set_pixel_jitter(0.0, 0.0)
    if seq == "at_rest":
        assert length[a] == 1 and length[b] == 1, (length[a], length[b])
        if kind == "temporal":  # (at rest the one tap is the pixel itself: nothing else restarts)
            others = filterable(gb["ids"])
            others[a] = others[b] = False
            assert (length[others] == 3).all()


@pytest.mark.parametrize("seq", sorted(TAA_SEQUENCES))
def test_temporal_history_drops_non_finite_values(tracer, guides, seq):
    _poisoned_sequence(tracer, guides, "temporal", seq, lib.temporal_params())


@pytest.mark.parametrize("seq", sorted(TAA_SEQUENCES))
@pytest.mark.parametrize("flags", TAA_FLAGS)
def test_taa_history_and_clamp_drop_non_finite_values(tracer, guides, flags, seq):
    _poisoned_sequence(tracer, guides, "taa", seq, lib.taa_params(flags=flags))
