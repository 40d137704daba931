"""What the ff_render_adaptive tests share: the planted sizes and sums of the tile error, and the mixed scene of the driver tests,
fixed on the CPU oracle (tests/test_adaptive_host.py asserts the mix on the reference alone)."""
import functools

import numpy as np

from gpupathtracer_amd import lib, scenes
from gpupathtracer_amd import types as T
import adaptive_ref as R

F = np.float32

# (width, height, tile): a tile of one pixel, a row and a column of 17, exactly 256 pixels, more than 256 with ragged right and
# bottom tiles, several lanes' worth per lane, a tile of 128
SIZES = [(1, 1, 16), (17, 1, 16), (1, 17, 16), (16, 16, 16), (17, 17, 16), (33, 31, 16), (257, 3, 32), (129, 130, 128)]
SIZE_IDS = [f"{w}x{h}_t{t}" for w, h, t in SIZES]
PASS_COUNTS = (2, 6, 1000)


def planted_sums(w, h, n, seed=0):
    """Random running sums after n passes: sum_even is about half of sum, so the errors are small and positive; a few pixels are
    black and a few have a negative or zero brightness."""
    rng = np.random.default_rng(1000 * w + h + 7 * n + seed)
    total = (rng.random((h, w, 3), dtype=F) * F(n) * F(0.8) + F(0.01)).astype(F)
    even = (total * F(0.5) * (F(1.0) + (rng.random((h, w, 3), dtype=F) - F(0.5)) * F(0.1))).astype(F)
    flat = rng.random((h, w)) < 0.1
    total[flat] = 0
    even[flat] = 0
    neg = rng.random((h, w)) < 0.05
    total[neg] = -total[neg]
    return total, even


def wide_sums(w, h, seed=5):
    """Running sums after 2 passes whose pixel errors span six orders of magnitude: the rounded sum of such a tile depends on the
    order of the adds (the balanced sums of planted_sums round to the same float in nearly any order)."""
    rng = np.random.default_rng(seed)
    total = (10.0 ** rng.uniform(-3, 3, (h, w, 3))).astype(F)
    even = (total * F(0.5) * (1 + 10.0 ** rng.uniform(-5, 0, (h, w, 3)))).astype(F)
    return total, even


# ---- the mixed scene of the driver tests ---------------------------------------------------------------------------------------
# A mesh on a floor under an area light, no environment: the tiles of the sky see only misses (error 0: they stop at the first
# check), the far floor is dim and quiet, the mesh and its shadow are not.  48 x 40 at tile 16 is a 3 x 3 grid whose bottom row is 8
# pixels tall.  The threshold is taken from the oracle's own tile errors at the first check (n = 2): it lies between them, so that
# with the errors of the later checks at least one tile stops at min_passes, one strictly between, and one runs to max_passes.
MIX_W, MIX_H, MIX_TILE = 48, 40, 16
MIX_SPP, MIX_BOUNCES, MIX_SEED = 2, 3, 1234
MIX_MIN, MIX_MAX = 2, 8
MIX_POSE = dict(position=(0.0, 0.5, 9.0), yaw=-90.0, pitch=8.0)
# The oracle's E_t at n = 2 are 0 for the six tiles that are still black, 0.01691 for the centre tile (the mesh under the light),
# 0.01599 and 0.01971 for the two tiles of the lit floor below it.  The threshold is three quarters of the centre tile's: the black
# tiles stop at n = 2, the centre tile's error falls to 0.01225 at n = 4 (it stops there), and the lit floor's grows (0.028, 0.036:
# more of its pixels have found the light) and runs to max_passes.
MIX_THRESHOLD = 0.0127
# With next-event estimation, which the oracle does not render, the same rule on the frames of Tracer.render_tile: the centre tile's
# E_t at n = 2 is 0.02059, three quarters of it 0.0154.  (Under 0.0127 the centre tile's 0.0144, 0.0134, 0.01165 at n = 4, 6, 8
# never fall below the threshold before max_passes, and no tile stops in between.)  The test asserts the mix on what the GPU returns.
MIX_THRESHOLD_NEE = 0.0154


def mix_scene():
    return scenes.open_floor_scene(area_light=True)


def mix_camera():
    return scenes.posed_camera(MIX_W, MIX_H, **MIX_POSE)


def mix_params(shade=T.SHADE_DIFFUSE_PATH, seed=MIX_SEED):
    return lib.render_params(MIX_W, MIX_H, MIX_BOUNCES, MIX_SPP, seed, shade_mode=shade)


def mix_adaptive(**overrides):
    fields = dict(tile=MIX_TILE, min_passes=MIX_MIN, max_passes=MIX_MAX, threshold=MIX_THRESHOLD)
    fields.update(overrides)
    return lib.adaptive_params(**fields)


class CachedRender:
    """A render callback for adaptive_ref.drive that renders every seed's whole frame once and cuts the rectangles out of it - a
    rectangle of the frame is the frame's pixels bit for bit (ff_render_tile's contract, which its own tests hold) - so that the
    reference is computed once and shared.  full(seed) -> float32 [H, W, 3]."""

    def __init__(self, full):
        self.full = functools.lru_cache(maxsize=None)(full)

    def __call__(self, seed, x0, y0, w, h):
        return self.full(seed)[y0:y0 + h, x0:x0 + w]


@functools.lru_cache(maxsize=None)
def oracle_frames():
    """The oracle's frames of the mixed scene in the path mode, by seed."""
    from oracle_lib import oracle_render
    scene, cam = mix_scene(), mix_camera()
    return CachedRender(lambda seed: oracle_render(scene, cam, mix_params(seed=seed), threads=8)[1])


@functools.lru_cache(maxsize=None)
def oracle_drive(guard=False, threshold=None):
    return R.drive(oracle_frames(), MIX_W, MIX_H, MIX_SEED, MIX_TILE, MIX_MIN, MIX_MAX, MIX_THRESHOLD if threshold is None else threshold, guard=guard)


def assert_mixed(tile_passes):
    """At least one tile stops at min_passes, one strictly between min_passes and max_passes, one runs to max_passes."""
    n = np.asarray(tile_passes)
    assert (n == MIX_MIN).any() and ((n > MIX_MIN) & (n < MIX_MAX)).any() and (n == MIX_MAX).any(), n
