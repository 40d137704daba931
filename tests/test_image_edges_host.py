"""The vectorised float64 references (gbuffer_ref.denoise_ref, temporal_ref.TemporalRef, taa_ref.TaaRef) against the loop-per-pixel
versions of tests/loop_ref.py at one-pixel rows and columns, tiny images, changes of size and non-finite pixels, on synthetic
G-buffers: several geometries, misses, emitters and mirrors, zero-length normals, coincident positions, zero albedo channels and
ids that name no geometry of the scene.  The references' array shifts, masks and padding are what goes wrong at such edges; the
GPU tests trust them.  No GPU: ff_camera_ray_matrix is a host function."""
import numpy as np
import pytest

from gpupathtracer_amd import lib, scenes
from gpupathtracer_amd import types as T
from gbuffer_ref import denoise_ref, filterable
from loop_ref import TaaLoop, TemporalLoop, denoise_loop
from taa_ref import TaaRef
from temporal_ref import TemporalRef

SIZES = [(1, 1), (1, 7), (7, 1), (3, 2), (12, 12)]  # (width, height)
DENOISE_FLAGS = [0, T.DENOISE_SAME_GEOMETRY, T.DENOISE_SAME_GEOMETRY | T.DENOISE_DEMODULATE_ALBEDO]
TAA_FLAGS = [0, T.TAA_BILINEAR, T.TAA_NO_CLAMP, T.TAA_BILINEAR | T.TAA_NO_CLAMP]
Z_WALL = -2.5
UNKNOWN = 7  # an id that names no geometry of MODELS


def translation(x, y, z):
    m = np.eye(4)
    m[:3, 3] = (x, y, z)
    inv = np.eye(4)
    inv[:3, 3] = (-x, -y, -z)
    return m, inv


MODELS = [translation(0, 0, 0), translation(0, 0, 0), translation(0, 0, 0)]
MOVED = [translation(0, 0, 0), translation(0.05, -0.03, 0.0), translation(0, 0, 0)]


def cam_at(w, h, k):
    """Poses about one pixel apart at 12x12 (a wall 4.9 units away)."""
    return scenes.posed_camera(w, h, position=(0.11 * k, -0.07 * k, 2.4), yaw=-90.0 + 0.4 * k, pitch=0.0)


def synthetic_gbuffer(camera, w, h, seed, jx=0.0, jy=0.0):
    """A wall filling the view (traced in float64 through the jittered pixel), split into geometries 0-2 with a tilted part, plus
    one each (where the image has room) of: a miss, an emitter, a mirror, a zero-length normal, a position equal to its left
    neighbour's, zero albedo channels and an id that names no geometry."""
    from temporal_ref import ray_matrix
    rng = np.random.default_rng(seed)
    M = ray_matrix(camera)
    eye = np.array([camera.m_position.x, camera.m_position.y, camera.m_position.z])
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    f = np.float64(np.float32(camera.m_farClip))
    px = (xs + jx) / camera.m_screenWidth * 2 - 1
    py = 1 - (ys + jy) / camera.m_screenHeight * 2
    d = (np.stack([px * f, py * f, np.full_like(px, f), np.full_like(px, f)], -1) @ M.T)[..., :3] - eye
    pos = eye + ((Z_WALL - eye[2]) / d[..., 2])[..., None] * d
    nrm = np.zeros((h, w, 3))
    nrm[..., 2] = 1.0
    ids = np.zeros((h, w, 3), np.int32)
    ids[..., 1] = -1
    ids[..., 2] = T.BXDF_DIFFUSE
    ids[:, w // 2:, 0] = 1
    ids[h // 2:, :, 0] = 2
    tilt = ids[..., 0] == 2  # geometry 2 is tilted: its normal leans and its points rise with x
    nrm[tilt] = (0.3, 0.0, 0.95)
    pos[tilt, 2] += -0.3 / 0.95 * (pos[tilt, 0] - pos[tilt, 0].min(initial=0.0))
    alb = rng.uniform(0.2, 0.9, size=(h, w, 3))
    flat = rng.permutation(w * h)
    special = [tuple(np.unravel_index(i, (h, w))) for i in flat[:7]] if w * h >= 8 else []
    for kind, at in zip(("miss", "emitter", "mirror", "zero_normal", "coincident", "zero_albedo", "unknown"), special):
        if kind == "miss":
            ids[at] = -1
            pos[at] = nrm[at] = alb[at] = 0.0
        elif kind == "emitter":
            ids[at + (2,)] = T.BXDF_EMITTER
        elif kind == "mirror":
            ids[at + (2,)] = T.BXDF_MIRROR
        elif kind == "zero_normal":
            nrm[at] = 0.0
        elif kind == "coincident" and at[1] > 0:
            pos[at] = pos[at[0], at[1] - 1]
        elif kind == "zero_albedo":
            alb[at + (0,)] = 0.0
            alb[at + (2,)] = 0.0
        elif kind == "unknown":
            ids[at + (0,)] = UNKNOWN
    return {"position": pos.astype(np.float32), "normal": nrm.astype(np.float32), "albedo": alb.astype(np.float32), "ids": ids}


def radiance(w, h, seed, poison=False):
    rng = np.random.default_rng(seed)
    rad = (rng.uniform(0.05, 2.0, size=(h, w, 3)) * np.where(rng.random((h, w, 1)) < 0.1, 6.0, 1.0)).astype(np.float32)
    bad = np.zeros((h, w), bool)
    if poison:
        cells = rng.permutation(w * h)[:2]
        for v, c in zip((np.nan, np.inf), cells):
            rad[np.unravel_index(c, (h, w))] = v
            bad[np.unravel_index(c, (h, w))] = True
    return rad, bad


def assert_same(loop, vec, skip, what):
    """Equal to 1e-9 (relative) wherever skip is False; there the outputs are also finite (ff_api.h's rule for non-finite input)."""
    keep = ~skip
    assert np.isfinite(vec[keep]).all() and np.isfinite(loop[keep]).all(), what
    np.testing.assert_allclose(vec[keep], loop[keep], rtol=1e-9, atol=1e-12, err_msg=what)


@pytest.mark.parametrize("poison", [False, True])
@pytest.mark.parametrize("flags", DENOISE_FLAGS)
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_denoise_ref_matches_the_loop(size, flags, poison):
    w, h = size
    gb = synthetic_gbuffer(cam_at(w, h, 0), w, h, seed=w * 31 + h)
    rad, bad = radiance(w, h, 7, poison)
    for iterations, sigma_color in ((1, 4.0), (3, 0.5), (5, 4.0)):
        args = (iterations, sigma_color, 0.1, 0.1, flags)
        vec, loop = denoise_ref(rad, gb, *args), denoise_loop(rad, gb, *args)
        assert_same(loop, vec, bad, f"{size} {args}")
        if poison:
            # every other pixel's output is what it is when the non-finite pixels are misses
            missed = dict(gb, ids=np.where(bad[..., None], -1, gb["ids"]))
            assert np.array_equal(vec[~bad], denoise_ref(rad, missed, *args)[~bad])


def _sequence(w_h_list, poison_at):
    """(size, pose, poison) per call: the sizes in turn, three calls each (pose 0, 1, 1), the poisoned call at the given index."""
    calls = []
    for (w, h) in w_h_list:
        for k in (0, 1, 1):
            calls.append(((w, h), k, len(calls) == poison_at))
    return calls


SEQUENCES = {
    "sizes": [(12, 12), (1, 7), (7, 1), (12, 12), (3, 2), (1, 1), (12, 12)],
    "tiny": [(1, 1), (3, 2)],
}


def run_pair(ref, loop, step_args, calls, moved_at=None, rest=False):
    for i, ((w, h), k, poison) in enumerate(calls):
        pose = 0 if rest else k
        c = cam_at(w, h, pose)
        gb = step_args["gbuffer"](c, w, h, i)
        rad, bad = radiance(w, h, 100 + i, poison)
        models = MOVED if moved_at is not None and i >= moved_at else MODELS
        r, q = ref.step(rad, gb, c, models, step_args["params"]), loop.step(rad, gb, c, models, step_args["params"])
        what = f"call {i} {w}x{h} pose {pose}"
        assert_same(q["out"], r["out"], bad, what)
        np.testing.assert_allclose(r["motion"], q["motion"], rtol=1e-9, atol=1e-9, err_msg=what)
        assert np.array_equal(r["length"], q["length"]), what
        if "valid" in q:
            assert np.array_equal(r["valid"], q["valid"]), what
        yield i, gb, bad, r


TEMPORAL_CASES = {
    "default": {},
    "accumulate": dict(iterations=0, feedback_pass=-1),
    "feedback_last": dict(iterations=3, feedback_pass=2, flags=T.DENOISE_SAME_GEOMETRY),
    "no_flags_short_history": dict(iterations=2, feedback_pass=-1, flags=0, max_history=2, variance_history=1),
    "long_variance_history": dict(iterations=1, feedback_pass=0, variance_history=20, reuse_normal=-1.0),
    "strict_reuse": dict(iterations=1, feedback_pass=0, reuse_normal=1.0, reuse_plane=0.0),
}


@pytest.mark.parametrize("rest", [False, True], ids=["moving", "at_rest"])
@pytest.mark.parametrize("seq", sorted(SEQUENCES))
@pytest.mark.parametrize("case", sorted(TEMPORAL_CASES))
def test_temporal_ref_matches_the_loop(case, seq, rest):
    tp = lib.temporal_params(**TEMPORAL_CASES[case])
    calls = _sequence(SEQUENCES[seq], poison_at=1)
    args = {"gbuffer": lambda c, w, h, i: synthetic_gbuffer(c, w, h, seed=w * 31 + h), "params": tp}
    for i, gb, bad, r in run_pair(TemporalRef(), TemporalLoop(), args, calls, moved_at=4):
        if i == 2:
            # the call after the poisoned one: all finite; at rest the poisoned pixels start afresh
            assert np.isfinite(r["out"]).all()
            if rest:
                hit = filterable(gb["ids"]) & (gb["ids"][..., 0] < len(MODELS))
                poisoned = _poisoned_cells(calls, 1)
                assert (r["length"][poisoned & hit] == 1).all()


def _poisoned_cells(calls, index):
    (w, h), _, _ = calls[index]
    return radiance(w, h, 100 + index, True)[1]


@pytest.mark.parametrize("rest", [False, True], ids=["moving", "at_rest"])
@pytest.mark.parametrize("seq", sorted(SEQUENCES))
@pytest.mark.parametrize("flags", TAA_FLAGS)
def test_taa_ref_matches_the_loop(flags, seq, rest):
    p = lib.taa_params(flags=flags, alpha_min=0.2, gamma=1.25)
    calls = _sequence(SEQUENCES[seq], poison_at=1)
    args = {"gbuffer": lambda c, w, h, i: synthetic_gbuffer(c, w, h, seed=w * 31 + h, jx=(i % 4) / 4.0, jy=((i * 3) % 4) / 4.0),
            "params": p}
    for i, gb, bad, r in run_pair(TaaRef(), TaaLoop(), args, calls, moved_at=4, rest=rest):
        if i == 2:
            assert np.isfinite(r["out"]).all()
            if rest:
                assert (r["length"][_poisoned_cells(calls, 1)] == 1).all()


def test_taa_clamp_box_leaves_out_non_finite_samples():
    """A +Inf pixel in the current frame leaves its neighbours' clamp box finite: mean, spread and bounds over the other eight."""
    from taa_ref import neighbourhood_box
    rng = np.random.default_rng(4)
    c = rng.uniform(0.1, 1.0, size=(5, 6, 3))
    lo, hi = neighbourhood_box(c, 1.0)
    bad = c.copy()
    bad[2, 3] = (np.inf, 0.5, 0.5)
    with np.errstate(invalid="ignore"):
        blo, bhi = neighbourhood_box(bad, 1.0)
    assert np.isfinite(blo).all() and np.isfinite(bhi).all()
    far = np.ones((5, 6), bool)
    far[1:4, 2:5] = False
    assert np.array_equal(blo[far], lo[far]) and np.array_equal(bhi[far], hi[far])
    # the pixel left of it: the box of its eight finite samples
    from taa_ref import YCOCG
    taps = np.array([c[y, x] for y in (1, 2, 3) for x in (1, 2, 3) if (y, x) != (2, 3)]) @ YCOCG.T
    mu, sd = taps.mean(0), np.sqrt(np.maximum(0.0, (taps * taps).mean(0) - taps.mean(0) ** 2))
    assert np.allclose(blo[2, 2], np.maximum(taps.min(0), mu - sd), rtol=1e-12) and np.allclose(bhi[2, 2], np.minimum(taps.max(0), mu + sd), rtol=1e-12)
