"""ff_upscale and ff_taa_upscale on the GPU at the edges their 160x90 comparisons do not reach.

ff_upscale (64x4 workgroups, one thread per high pixel), on the scene-free view of tests/upscale_views.py: low images of one pixel,
one row and one column, factors 1 and 8, ratios that differ along the axes, high images narrower than a wave row and lower than a
workgroup, both jitters, sigmas far from the defaults, zero-length guide normals and 1920x1080, against the float64 reference
(tests/upscale_ref.py) and the host twin; and what holds bit for bit without a reference: the identity at equal sizes, a constant
colour, power-of-two scaling.

ff_taa_upscale (16x16 tiles, a low footprint of up to 20x20 pixels staged in LDS), on real G-buffers of cornell_wahoo_scene:
equal sizes under a jitter (the widest footprint), factor 8 and ratios near it (the narrowest), tiles cut by the right and the
bottom edge over a low image of one or two pixels, alpha_min and gamma far from the defaults, against TaaUpscaleRef under the
tolerances of test_gpu_taa_upscale.py; and bit for bit: ff_taa at equal sizes without jitter, the exact rebuild of an image from a
cycle of jittered low frames at factors 2 and 4, power-of-two scaling.

The size pair (65,33) -> (257,33) of the ff_upscale cases is not run through ff_taa_upscale: the camera's horizontal field of view
follows the aspect ratio, so a 65x33 and a 257x33 frame of one pose show different frusta, ids_lo seldom matches and nearly every
pixel takes the spatial estimate.  (The pairs whose aspects differ by a rounding, such as (21,12) -> (161,91), stay: the operator is
defined for any two G-buffers, and the reference is given the same ones.)"""
import functools

import numpy as np
import pytest

from gpupathtracer_amd import lib, scenes
from gpupathtracer_amd import types as T
from gbuffer_ref import rgb8_of
from taa_upscale_ref import BLEND, FIRST, HOLD, SPATIAL, TaaUpscaleRef
from temporal_ref import scene_models
from upscale_ref import STEP_2X2, STEP_FALLBACK, upscale_ref
from upscale_views import (EDGE_FLAGS, EDGE_JITTERS, EDGE_PAIRS, EDGE_SIGMAS, SCALING_EXPONENT, noisy_radiance, pair_id, view,
                           zero_normal_patch)

pytestmark = pytest.mark.gpu

HD = ((960, 540), (1920, 1080))
SCALING_PAIRS = [((21, 12), (161, 91)), ((9, 7), (65, 35))]
SHARE_MIN_PIXELS = 1000  # test_gpu_image_edges.py's rule: a share bound applies from this many pixels on


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def largest_error(out, ref):
    """The largest relative error over the values whose reference is above 1e-3 (test_gpu_upscale.assert_matches' figure)."""
    big = np.abs(ref) > 1e-3
    return float((np.abs(np.asarray(out, np.float64) - ref)[big] / np.abs(ref)[big]).max(initial=0.0))


# ---- ff_upscale ---------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=64)
def edge_case(pair, jitters, zero_normal=False):
    """(low view, high view, low radiance) of one size pair under one (lo, hi) jitter pair; shared, never written to."""
    (w, h), (W, H) = pair
    lo, hi = view(w, h, jitters[0], zero_normal), view(W, H, jitters[1], zero_normal)
    return lo, hi, noisy_radiance(lo)


def check_upscale(tracer, lo, hi, rad, p):
    """One ff_upscale call against upscale_ref and ff_upscale_host, both at 1e-4 -> (out, reference's steps, the two errors)."""
    lo_j, hi_j = tuple(p.lo_jitter), tuple(p.hi_jitter)
    out8, out = tracer.upscale(rad, lo, hi, p)
    ref, steps = upscale_ref(rad, lo, hi, p.sigma_normal, p.sigma_plane, p.flags, lo_j, hi_j)
    _, host = lib.upscale_host(rad, lo, hi, p)
    e_ref, e_host = largest_error(out, ref), largest_error(out, host.astype(np.float64))
    what = (lo_j, hi_j, p.sigma_normal, p.sigma_plane)
    assert np.isfinite(out).all(), what
    assert e_ref <= 1e-4, (what, e_ref)
    assert e_host <= 1e-4, (what, e_host)
    assert np.array_equal(out8, rgb8_of(out)), what
    return out, steps, e_ref, e_host


@pytest.mark.parametrize("flags", EDGE_FLAGS)
@pytest.mark.parametrize("pair", EDGE_PAIRS, ids=pair_id)
def test_upscale_matches_the_reference_and_the_host_twin_at_edge_sizes(tracer, pair, flags):
    """The whole product of test_upscale_host.py's edge cases: every jitter pair and sigma pair at every size pair and flag set.  The
    two sides differ only in expf."""
    worst_ref = worst_host = 0.0
    for jitters in EDGE_JITTERS:
        lo, hi, rad = edge_case(pair, jitters)
        for sn, sp in EDGE_SIGMAS:
            p = lib.upscale_params(flags=flags, sigma_normal=sn, sigma_plane=sp, lo_jitter=jitters[0], hi_jitter=jitters[1])
            _, _, e_ref, e_host = check_upscale(tracer, lo, hi, rad, p)
            worst_ref, worst_host = max(worst_ref, e_ref), max(worst_host, e_host)
    print(f"ff_upscale {pair_id(pair)} flags {flags}: largest relative error vs reference {worst_ref:.3g}, vs host twin {worst_host:.3g}")


@pytest.mark.parametrize("flags", EDGE_FLAGS)
@pytest.mark.parametrize("pair", SCALING_PAIRS, ids=pair_id)
def test_upscale_matches_the_reference_on_zero_length_normals(tracer, pair, flags):
    """test_upscale_host.py's zero-normal view: inv = 0 for the pixel and for a tap, a_n = 1 / sigma_normal (past the cut-off at
    sigma_normal 0.0125, where the patch falls through both rounds to the nearest low pixel)."""
    worst_ref = worst_host = 0.0
    for jitters in EDGE_JITTERS:
        lo, hi, rad = edge_case(pair, jitters, True)
        assert zero_normal_patch(lo).sum() >= 2 and zero_normal_patch(hi).sum() >= 20
        for sn, sp in EDGE_SIGMAS[:3]:
            p = lib.upscale_params(flags=flags, sigma_normal=sn, sigma_plane=sp, lo_jitter=jitters[0], hi_jitter=jitters[1])
            _, steps, e_ref, e_host = check_upscale(tracer, lo, hi, rad, p)
            worst_ref, worst_host = max(worst_ref, e_ref), max(worst_host, e_host)
            assert (steps[zero_normal_patch(hi)] == (STEP_FALLBACK if sn == 0.0125 else STEP_2X2)).all()
    print(f"ff_upscale zero normals {pair_id(pair)} flags {flags}: largest relative error vs reference {worst_ref:.3g}, vs host twin {worst_host:.3g}")


@pytest.mark.parametrize("size", [(1, 1), (7, 5), (65, 5), (257, 33)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_upscale_at_equal_sizes_returns_the_image(tracer, size):
    gb = view(*size)
    rad = noisy_radiance(gb)
    out8, out = tracer.upscale(rad, gb, gb, lib.upscale_params(flags=T.DENOISE_SAME_GEOMETRY))
    assert np.array_equal(bits(out), bits(rad))
    assert np.array_equal(out8, rgb8_of(out))


@pytest.mark.parametrize("flags", EDGE_FLAGS[:2])
@pytest.mark.parametrize("pair", EDGE_PAIRS, ids=pair_id)
def test_upscale_returns_a_constant_colour_bit_for_bit(tracer, pair, flags):
    """UpscaleMean's guarantee: c_0 + sum w (c_q - c_0) / sum w is c_0 when every tap holds c_0, and step 4 hands the low pixel on
    as it is: every high pixel, filterable or not, fallback or not, under every jitter."""
    colour = np.array([0.3, 1.7, 0.011], dtype=np.float32)
    for jitters in EDGE_JITTERS:
        lo, hi, _ = edge_case(pair, jitters)
        rad = np.broadcast_to(colour, lo["position"].shape).copy()
        p = lib.upscale_params(flags=flags, lo_jitter=jitters[0], hi_jitter=jitters[1])
        out8, out = tracer.upscale(rad, lo, hi, p)
        assert np.array_equal(bits(out), bits(np.broadcast_to(colour, out.shape))), jitters
        assert np.array_equal(out8, rgb8_of(out))


@pytest.mark.parametrize("flags", EDGE_FLAGS)
@pytest.mark.parametrize("pair", SCALING_PAIRS, ids=pair_id)
def test_upscale_power_of_two_scaling_is_exact(tracer, pair, flags):
    """out(rad * s) == out(rad) * s bit for bit for s = 2^-20 and 2^20.  The exponent is the one at which the host twin holds exactly
    (test_upscale_host.py: test_power_of_two_scaling_is_exact_through_the_host_twin, on the same views and radiance): 20, because no
    product w (c - c_0) of noisy_radiance goes subnormal at 2^-20."""
    for jitters in EDGE_JITTERS:
        lo, hi, rad = edge_case(pair, jitters)
        p = lib.upscale_params(flags=flags, lo_jitter=jitters[0], hi_jitter=jitters[1])
        _, base = tracer.upscale(rad, lo, hi, p)
        for s in (np.float32(2.0 ** -SCALING_EXPONENT), np.float32(2.0 ** SCALING_EXPONENT)):
            _, scaled = tracer.upscale(rad * s, lo, hi, p)
            assert np.array_equal(bits(scaled), bits(base * s)), (jitters, float(s))


_HD_RUN = {}


def hd_run(tracer):
    """(low view, high view, radiance, GPU rgb8, GPU radiance) of the one 1080p call, default parameters; made once."""
    if not _HD_RUN:
        lo, hi = view(*HD[0]), view(*HD[1])
        rad = noisy_radiance(lo)
        _HD_RUN["run"] = (lo, hi, rad, *tracer.upscale(rad, lo, hi))
    return _HD_RUN["run"]


def test_upscale_1080p_matches_the_host_twin(tracer):
    lo, hi, rad, out8, out = hd_run(tracer)
    _, host = lib.upscale_host(rad, lo, hi)
    err = largest_error(out, host.astype(np.float64))
    print(f"ff_upscale {pair_id(HD)}: largest relative error vs host twin {err:.3g}")
    assert np.isfinite(out).all()
    assert err <= 1e-4, err
    assert np.array_equal(out8, rgb8_of(out))


@pytest.mark.parametrize("band", [(y, y + 180) for y in range(0, HD[1][1], 180)], ids=lambda b: f"rows{b[0]}-{b[1]}")
def test_upscale_1080p_matches_the_reference(tracer, band):
    """The float64 reference takes a quarter of a minute at this size: it is compared a band of 180 rows at a time."""
    lo, hi, rad, _, out = hd_run(tracer)
    ref, steps = upscale_ref(rad, lo, hi, rows=band)
    err = largest_error(out[band[0]:band[1]], ref)
    print(f"ff_upscale {pair_id(HD)} rows {band}: largest relative error vs reference {err:.3g}, 2x2 share {(steps == STEP_2X2).mean():.4f}")
    assert err <= 1e-4, err


# ---- ff_taa_upscale ----------------------------------------------------------------------------------------------------------

SCENE = "cornell_wahoo_scene"
# test_gpu_taa_upscale.py's poses and sequences (copied, not imported)
POSES = [((0.0, 0.0, 2.4), -90.0), ((0.06, -0.04, 2.4), -89.3), ((0.1, -0.02, 2.37), -88.8)]
TAA_SEQUENCES = {"at_rest": (0, 0, 0), "sliding": (0, 1, 2)}
TAA_FLAGS = [0, T.TAA_BILINEAR, T.TAA_NO_CLAMP, T.TAA_BILINEAR | T.TAA_NO_CLAMP]
# (low, high): one low pixel under one tile and under a cut tile; one or two low pixels under tiles cut on both edges; factor ~2
# with cut tiles; equal sizes (under jitter_of(1) and jitter_of(2) the footprint is the widest: 19 of the 20 staged columns from
# ox = -2), small and over several tiles; factor 8 (the narrowest footprint) and non-integer factors just below it
TAA_PAIRS = [((1, 1), (1, 1)), ((1, 1), (8, 8)), ((2, 3), (15, 17)), ((9, 9), (17, 17)), ((17, 15), (17, 15)), ((161, 91), (161, 91)),
             ((20, 12), (160, 96)), ((21, 12), (161, 91))]
TAA_PARAM_PAIRS = [((21, 12), (161, 91)), ((17, 15), (17, 15))]
TAA_PARAMS = {"alpha_min_1": dict(alpha_min=1.0), "alpha_min_0.01": dict(alpha_min=0.01), "gamma_0.05": dict(gamma=0.05),
              "gamma_100": dict(gamma=100.0)}
CASES_SEEN = set()  # step 6's cases over every reference comparison of this module (test_every_blend_case_was_compared)


def cam(pose, w, h):
    (x, y, z), yaw = POSES[pose]
    return scenes.posed_camera(w, h, position=(x, y, z), yaw=yaw, pitch=0.0)


def synthetic_radiance(seed, w, h):
    """test_gpu_temporal's seeded radiance: a smooth image times noise, a few pixels far brighter than their neighbours (every
    channel in [0.03, 10])."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    smooth = np.stack([0.4 + 0.3 * np.sin(xx / 17.0), 0.3 + 0.2 * np.cos(yy / 11.0), 0.2 + 0.001 * xx], -1)
    rad = smooth * rng.uniform(0.3, 1.7, size=(h, w, 3)) * np.where(rng.random((h, w, 1)) < 0.02, 8.0, 1.0)
    return rad.astype(np.float32)


@functools.lru_cache(maxsize=None)
def the_scene():
    return getattr(scenes, SCENE)()


def jitter_of(i):
    return lib.jitter_sequence(i, 16)


@pytest.fixture(scope="module")
def guides():
    """guides(pose, w, h, jitter=(0, 0)): ff_gbuffer of the scene at that pose, size and jitter, from one Tracer of the module's own
    (the tracer under test keeps its state); images up to 161x91 are cached."""
    own, cache = [], {}

    def get(pose, w, h, jitter=(0.0, 0.0)):
        key = (pose, w, h, tuple(jitter))
        if key in cache:
            return cache[key]
        if not own:
            own.append(lib.Tracer(0))
            own[0].upload_scene(the_scene())
        t = own[0]
        t.set_pixel_jitter(*jitter)
        try:
            gb = t.gbuffer(cam(pose, w, h), lib.render_params(w, h))
        finally:
            t.set_pixel_jitter(0.0, 0.0)
        if w * h <= 161 * 91:
            cache[key] = gb
        return gb

    yield get
    for t in own:
        t.close()


def check_taa_upscale(tracer, guides, pair, seq, **over):
    """One three-call ff_taa_upscale sequence against TaaUpscaleRef under test_gpu_taa_upscale.test_matches_the_numpy_reference's
    rules: call i on synthetic_radiance(100 + i) with the low G-buffer under jitter_of(i).  Sliding, the output and motion tolerances
    grow with the image past 160 pixels (test_gpu_image_edges.check_taa: the float32 error of a pixel coordinate is relative to it,
    and the resampled history moves with it).  The excused-share caps apply from SHARE_MIN_PIXELS high pixels on; below, every pixel
    that is not excused is still compared."""
    (w, h), (W, H) = pair
    over = dict(dict(alpha_min=0.2, gamma=1.25), **over)
    tracer.upload_scene(the_scene())
    tracer.taa_upscale_reset()
    ref, models = TaaUpscaleRef(), scene_models(the_scene())
    grow = max(1.0, W / 160.0) if seq == "sliding" else 1.0
    tol, motion_tol = 1e-3 * grow, 2e-3 * grow
    for i, k in enumerate(TAA_SEQUENCES[seq]):
        j = jitter_of(i)
        p = lib.taa_upscale_params(lo_jitter=j, **over)
        g_lo, g_hi, c = guides(k, w, h, j), guides(k, W, H), cam(k, W, H)
        rad = synthetic_radiance(100 + i, w, h)
        _, out = tracer.taa_upscale(rad, g_lo, g_hi, c, p)
        motion, length = tracer.taa_upscale_history()
        r = ref.step(rad, g_lo["ids"], g_hi, c, models, p)
        excused = r["tainted"]
        err = (np.abs(out.astype(np.float64) - r["out"]) / np.maximum(np.abs(r["out"]), 0.1)).max(-1)
        merr = np.abs(motion - r["motion"]).max(-1)
        lerr = np.abs(length - r["length"]) / np.maximum(r["length"], 1e-30)
        e, me, le = (float(v[~excused].max(initial=0.0)) for v in (err, merr, lerr))
        counts = np.bincount(r["case"].ravel(), minlength=4)
        print(f"ff_taa_upscale {seq} {pair_id(pair)} {over} flags {p.flags} call {i}: max rel err {e:.3g}, motion err {me:.3g}, length err {le:.3g}, "
              f"excused share {excused.mean():.4f}, valid {r['valid'].mean():.3f}, cases {counts}")
        CASES_SEEN.update(int(v) for v in np.unique(r["case"]))
        if W * H >= SHARE_MIN_PIXELS:
            assert excused.mean() <= (0.0 if seq == "at_rest" else 0.1), excused.mean()
        assert e <= tol, (i, e, np.argwhere((err > tol) & ~excused)[:5])
        assert me <= motion_tol, (i, me)
        assert le <= 1e-6, (i, le)
        if seq == "at_rest":
            assert not motion.any()


@pytest.mark.parametrize("seq", sorted(TAA_SEQUENCES))
@pytest.mark.parametrize("flags", TAA_FLAGS)
@pytest.mark.parametrize("pair", TAA_PAIRS, ids=pair_id)
def test_taa_upscale_matches_the_reference_at_edge_sizes(tracer, guides, pair, flags, seq):
    check_taa_upscale(tracer, guides, pair, seq, flags=flags)


@pytest.mark.parametrize("seq", sorted(TAA_SEQUENCES))
@pytest.mark.parametrize("case", sorted(TAA_PARAMS))
@pytest.mark.parametrize("pair", TAA_PARAM_PAIRS, ids=pair_id)
def test_taa_upscale_parameters_match_the_reference(tracer, guides, pair, case, seq):
    check_taa_upscale(tracer, guides, pair, seq, **TAA_PARAMS[case])


def test_every_blend_case_was_compared(tracer, guides):
    """BLEND, HOLD, FIRST and SPATIAL each occurred in a reference comparison above (run on its own, in two of them here)."""
    if not CASES_SEEN:
        for seq in sorted(TAA_SEQUENCES):
            check_taa_upscale(tracer, guides, TAA_PARAM_PAIRS[0], seq)
    assert CASES_SEEN == {BLEND, HOLD, FIRST, SPATIAL}, CASES_SEEN


def same_bits(x, y):
    return np.array_equal(x[0], y[0]) and all(np.array_equal(bits(u), bits(v)) for u, v in zip(x[1:], y[1:]))


def taa_and_taa_upscale_agree(tracer, guides, size, seq, flags):
    """Three calls of ff_taa and of ff_taa_upscale at equal sizes with lo_jitter 0 on the same inputs: (rgb8, radiance, motion,
    length) equal bit for bit; returns the last lengths."""
    w, h = size
    tracer.upload_scene(the_scene())
    tracer.taa_reset()
    tracer.taa_upscale_reset()
    for i, k in enumerate(TAA_SEQUENCES[seq]):
        gb, c = guides(k, w, h, jitter_of(i)), cam(k, w, h)
        rad = synthetic_radiance(100 + i, w, h)
        a = tracer.taa(rad, gb, c, lib.taa_params(flags=flags, alpha_min=0.2, gamma=1.25)) + tracer.taa_history()
        b = tracer.taa_upscale(rad, gb, gb, c, lib.taa_upscale_params(flags=flags, alpha_min=0.2, gamma=1.25)) + tracer.taa_upscale_history()
        assert same_bits(a, b), i
    return a[3]


@pytest.mark.parametrize("flags", TAA_FLAGS)
@pytest.mark.parametrize("size", [(1, 1), (1, 37), (37, 1), (15, 17), (65, 5), (257, 33)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_taa_upscale_at_equal_sizes_without_jitter_is_ff_taa_bit_for_bit(tracer, guides, size, flags):
    taa_and_taa_upscale_agree(tracer, guides, size, "sliding", flags)


def test_taa_upscale_at_equal_sizes_without_jitter_is_ff_taa_bit_for_bit_at_1080p(tracer, guides):
    length = taa_and_taa_upscale_agree(tracer, guides, HD[1], "at_rest", 0)
    assert (length == 3).all()


@pytest.mark.parametrize("flags", [T.TAA_NO_CLAMP, T.TAA_NO_CLAMP | T.TAA_BILINEAR])
@pytest.mark.parametrize("hi,factor", [((66, 34), 2), ((68, 36), 4)], ids=["66x34_factor_2", "68x36_factor_4"])
def test_a_cycle_of_low_frames_rebuilds_the_image_exactly_where_tiles_are_cut(tracer, guides, hi, factor, flags):
    """test_gpu_taa_upscale's exact rebuild at sizes whose last tiles are cut on both edges, and at factor 4: low frame (a, b) is
    target[b::F, a::F] under lo_jitter (a/F, b/F).  u = (X w) / W - a/F is exactly (X - a) / F in float32 and k is 1 on a pixel's own
    sample and 0 elsewhere, so after F^2 calls every pixel is the target bit for bit with length 1, and a second cycle brings every
    length to 2 (test_taa_upscale_host.py shows it of the reference for both factors)."""
    W, H = hi
    F = factor
    tracer.upload_scene(the_scene())
    tracer.taa_upscale_reset()
    gb, c = guides(0, W, H), cam(0, W, H)
    target = np.random.default_rng(5).uniform(0.5, 1.0, size=(H, W, 3)).astype(np.float32)
    done = np.zeros((H, W), bool)
    for cycle in range(2):
        for b in range(F):
            for a in range(F):
                p = lib.taa_upscale_params(flags=flags, lo_jitter=(a / F, b / F))
                _, out = tracer.taa_upscale(target[b::F, a::F], {"ids": gb["ids"][b::F, a::F]}, gb, c, p)
                motion, length = tracer.taa_upscale_history()
                done[b::F, a::F] = True
                assert np.array_equal(bits(out[done]), bits(target[done])), (cycle, a, b)
                assert not motion.any()
        assert done.all() and np.array_equal(bits(out), bits(target))
        assert (length == cycle + 1).all(), (cycle, length.min(), length.max())


@pytest.mark.parametrize("scale", [2.0 ** -20, 2.0 ** 20], ids=["2^-20", "2^20"])
@pytest.mark.parametrize("flags", TAA_FLAGS)
def test_taa_upscale_power_of_two_scaling_is_exact(tracer, guides, flags, scale):
    """test_gpu_image_edges.test_power_of_two_scaling_is_exact's statement for ff_taa, whose motion, resampling and clamp code this
    kernel shares, at (81,46) -> (161,91): the radiance keeps every channel in [0.03, 10], so nothing the kernel computes from it is
    subnormal or overflows at either scale; every output is exactly the scaled output, motion and length keep their bits."""
    s = np.float32(scale)
    (w, h), (W, H) = (81, 46), (161, 91)
    tracer.upload_scene(the_scene())
    for seq in sorted(TAA_SEQUENCES):
        outs = []
        for k in (np.float32(1.0), s):
            tracer.taa_upscale_reset()
            calls = []
            for i, pose in enumerate(TAA_SEQUENCES[seq]):
                j = jitter_of(i)
                _, o = tracer.taa_upscale(synthetic_radiance(100 + i, w, h) * k, guides(pose, w, h, j), guides(pose, W, H), cam(pose, W, H),
                                          lib.taa_upscale_params(flags=flags, lo_jitter=j))
                calls.append((o, *tracer.taa_upscale_history()))
            outs.append(calls)
        for i, ((o1, m1, l1), (o2, m2, l2)) in enumerate(zip(*outs)):
            assert np.array_equal(bits(o2), bits(o1 * s)), (seq, i)
            assert np.array_equal(bits(m1), bits(m2)) and np.array_equal(bits(l1), bits(l2)), (seq, i)
