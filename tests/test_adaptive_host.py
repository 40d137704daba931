"""ff_render_adaptive on the host side: exports and defaults, the host twin of the tile error ff_adaptive_tile_error_host - the
kernel's inline functions compiled for the host - bit for bit against the numpy float32 restatement (tests/adaptive_ref.py) with its
fixed order of adds, the rectangle plan, every refused parameter, and the whole driver of the restatement over the CPU oracle on the
mixed scene the GPU tests use."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from gpupathtracer_amd import lib
from gpupathtracer_amd import types as T
import adaptive_ref as R
from adaptive_cases import (MIX_H, MIX_MAX, MIX_MIN, MIX_THRESHOLD, MIX_TILE, MIX_W, PASS_COUNTS, SIZE_IDS, SIZES, assert_mixed, oracle_drive,
                            oracle_frames, planted_sums, wide_sums)

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ff_adaptive_params_init", "ff_render_adaptive", "ff_adaptive_state", "ff_adaptive_tile_error", "ff_adaptive_tile_error_host",
       "ff_adaptive_plan_host")


def last_error():
    return lib.load().ff_last_error().decode()


def same_bits(a, b):
    return np.array_equal(R.bits(a), R.bits(b))


def test_new_entry_points_are_exported_and_declared(ff):
    handle = ff.load()
    header = open(os.path.join(ROOT, "include", "firefly", "ff_api.h")).read()
    declared = set(re.findall(r"FF_API\s+[\w\s\*]+?\b(ff_\w+)\s*\(", header))
    for name in NEW:
        assert name in ff.EXPORTS and name in declared and hasattr(handle, name), name


def test_adaptive_params_defaults_and_sizes():
    p = lib.adaptive_params()
    assert (p.tile, p.min_passes, p.max_passes, p.flags, p.reserved) == (64, 2, 64, 0, 0) and F(p.threshold) == F(0.0002)
    assert C.sizeof(T.FfAdaptiveParams) == T.ADAPTIVE_PARAMS_BYTES == 24 and C.sizeof(T.FfAdaptiveInfo) == T.ADAPTIVE_INFO_BYTES == 32
    types_h = open(os.path.join(ROOT, "include", "firefly", "ff_types.h")).read()
    assert "static_assert(sizeof(FfAdaptiveParams) == 24" in types_h and "_Static_assert(sizeof(FfAdaptiveParams) == 24" in types_h
    assert "static_assert(sizeof(FfAdaptiveInfo) == 32" in types_h and "_Static_assert(sizeof(FfAdaptiveInfo) == 32" in types_h
    assert re.search(r"#define\s+FF_ADAPTIVE_GUARD_NEIGHBOURS\s+1\b", types_h)
    assert lib.adaptive_params(tile=16, threshold=0.5).tile == 16
    with pytest.raises(TypeError):
        lib.adaptive_params(tiles=16)


# ---- the tile error ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("w,h,tile", SIZES, ids=SIZE_IDS)
def test_twin_equals_the_restatement_bit_for_bit(w, h, tile):
    for n in PASS_COUNTS:
        total, even = planted_sums(w, h, n)
        got = lib.adaptive_tile_error_host(total, even, tile, n)
        exp = R.tile_errors(total, even, tile, n)
        assert got.shape == exp.shape == R.tile_grid(w, h, tile)
        assert same_bits(got, exp), (n, got, exp)
        assert np.isfinite(exp).all() and ((exp > 0).any() or w * h < 64)  # (the inputs exercise the sum)


def test_equal_means_and_black_tiles_give_exactly_zero():
    w, h, tile, n = 33, 31, 16, 4
    rng = np.random.default_rng(3)
    even = rng.random((h, w, 3), dtype=F) + F(0.25)
    total = even * F(2.0)  # sum_even * (1 / 2) == sum * (1 / 4) exactly
    assert not lib.adaptive_tile_error_host(total, even, tile, n).any() and not R.tile_errors(total, even, tile, n).any()
    black = np.zeros((h, w, 3), F)
    assert not lib.adaptive_tile_error_host(black, black, tile, n).any()
    # one black tile among noisy ones: its error alone is 0
    total, even = planted_sums(w, h, n)
    total[16:32, 0:16] = 0
    even[16:32, 0:16] = 0
    got = lib.adaptive_tile_error_host(total, even, tile, n)
    assert same_bits(got, R.tile_errors(total, even, tile, n))
    assert got[1, 0] == 0 and np.count_nonzero(got) == got.size - 1


def test_a_negative_brightness_gives_zero():
    w, h, tile, n = 17, 17, 16, 2
    total = np.full((h, w, 3), -1.0, F)
    even = np.full((h, w, 3), 5.0, F)
    assert not lib.adaptive_tile_error_host(total, even, tile, n).any()
    # channels that cancel to d == 0, and to -0
    total[..., :] = (1.0, -1.0, 0.0)
    assert not lib.adaptive_tile_error_host(total, even, tile, n).any() and not R.tile_errors(total, even, tile, n).any()
    # a single pixel of positive brightness shows
    total[3, 4] = (1.0, 1.0, 1.0)
    got = lib.adaptive_tile_error_host(total, even, tile, n)
    assert same_bits(got, R.tile_errors(total, even, tile, n)) and got[0, 0] > 0 and np.count_nonzero(got) == 1


@pytest.mark.parametrize("which,poison", [(1, float("nan")), (0, float("inf")), (1, float("inf")), (1, float("-inf"))],
                         ids=["nan_in_sum_even", "inf_in_sum", "inf_in_sum_even", "-inf_in_sum_even"])
def test_a_non_finite_pixel_poisons_its_tile_only(which, poison):
    """A NaN of sum_even gives |I - NaN| = NaN; an infinite sum gives I = d = inf and inf / inf = NaN; an infinite sum_even gives
    inf / sqrt(d) = inf.  (A NaN of `sum` is the next test's.)"""
    w, h, tile, n = 33, 31, 16, 6
    total, even = planted_sums(w, h, n)
    total[20, 18] = np.abs(total[20, 18]) + F(1.0)  # tile (1, 1); a pixel of positive brightness
    clean = lib.adaptive_tile_error_host(total, even, tile, n)
    planes = [total.copy(), even.copy()]
    planes[which][20, 18, 1] = poison
    got = lib.adaptive_tile_error_host(planes[0], planes[1], tile, n)
    assert same_bits(got, R.tile_errors(planes[0], planes[1], tile, n))
    bad = ~np.isfinite(got)
    assert bad[1, 1] and bad.sum() == 1
    assert same_bits(got[~bad], clean[~bad])


def test_a_nan_brightness_counts_as_black():
    """The definition's e_p = 0 where !(d > 0) also takes a NaN d: a NaN in `sum` itself removes its pixel from the tile's error
    and poisons nothing (the radiance of that pixel is NaN all the same).  Twin and restatement agree on it."""
    w, h, tile, n = 33, 31, 16, 6
    total, even = planted_sums(w, h, n)
    total[20, 18] = np.abs(total[20, 18]) + F(1.0)
    clean = lib.adaptive_tile_error_host(total, even, tile, n)
    total[20, 18, 1] = np.nan
    got = lib.adaptive_tile_error_host(total, even, tile, n)
    assert same_bits(got, R.tile_errors(total, even, tile, n)) and np.isfinite(got).all()
    changed = ~(R.bits(got) == R.bits(clean))
    assert changed[1, 1] and changed.sum() == 1 and got[1, 1] < clean[1, 1]


def test_the_order_of_the_adds_is_the_specified_one():
    """A permutation of a tile's pixels that changes the float sum changes the twin (fed the permuted image) and the restatement
    (fed the permuted vector) alike - and the restatement under another order of adds, a plain left-to-right sum, disagrees."""
    w = h = tile = 32  # one tile of 1024 pixels: four per lane
    n = 2
    total, even = wide_sums(w, h)
    base = lib.adaptive_tile_error_host(total, even, tile, n)
    assert same_bits(base, R.tile_errors(total, even, tile, n))
    rng = np.random.default_rng(11)
    changed = 0
    for _ in range(8):
        perm = rng.permutation(w * h)
        t2 = total.reshape(-1, 3)[perm].reshape(h, w, 3)
        e2 = even.reshape(-1, 3)[perm].reshape(h, w, 3)
        got = lib.adaptive_tile_error_host(t2, e2, tile, n)
        exp = R.tile_errors(total, even, tile, n, order=lambda v: v[perm])
        assert same_bits(got, exp)
        changed += int(not same_bits(got, base))
    assert changed >= 4, "the permutations should change the rounded sum"
    e = R.pixel_errors(total, even, n).reshape(-1)
    serial = F(0.0)
    for v in e:
        serial = F(serial + v)
    assert not same_bits(R.scale(serial, e.size, w * h), base[0, 0]), "a serial sum is another order"
    # the order is the tile's row-major one, not the image's: a ragged tile's pixels are its own rows back to back
    total, even = wide_sums(40, 32, seed=9)
    got = lib.adaptive_tile_error_host(total, even, 32, n)
    right = R.pixel_errors(total, even, n)[:, 32:40].reshape(-1)
    assert same_bits(got[0, 1], R.scale(R.ordered_sum(right), right.size, 40 * 32))


def test_tile_error_refusals():
    total, even = planted_sums(17, 15, 2)
    out = np.zeros((1, 2), F)
    call = lambda w, h, tile, n, a, b, o: lib.load().ff_adaptive_tile_error_host(  # noqa: E731
        w, h, tile, n, a.ctypes.data if a is not None else None, b.ctypes.data if b is not None else None, o.ctypes.data if o is not None else None)
    assert call(17, 15, 16, 2, total, even, out) == T.FF_OK
    for args, word in [((0, 15, 16, 2, total, even, out), "size"), ((17, 70000, 16, 2, total, even, out), "size"), ((17, 15, 8, 2, total, even, out), "tile"),
                       ((17, 15, 48, 2, total, even, out), "tile"), ((17, 15, 16, 3, total, even, out), "n must"), ((17, 15, 16, 0, total, even, out), "n must"),
                       ((17, 15, 16, 65536, total, even, out), "n must"), ((17, 15, 16, 2, None, even, out), "sum is null"),
                       ((17, 15, 16, 2, total, None, out), "sum_even"), ((17, 15, 16, 2, total, even, None), "out_error")]:
        assert call(*args) == T.FF_ERR_INVALID_ARG and word in last_error(), (word, last_error())


# ---- the plan ------------------------------------------------------------------------------------------------------------------

def check_plan(active):
    active = np.asarray(active, dtype=bool)
    got = lib.adaptive_plan_host(active)
    assert np.array_equal(got, R.plan(active)), (got, R.plan(active))
    cover = np.zeros(active.shape, dtype=np.int32)
    for tx0, ty0, tx1, ty1 in got:
        assert 0 <= tx0 < tx1 <= active.shape[1] and 0 <= ty0 < ty1 <= active.shape[0]
        cover[ty0:ty1, tx0:tx1] += 1
    assert np.array_equal(cover, active.astype(np.int32)), "disjoint, and exactly the active tiles"
    return got


def test_plan_shapes():
    assert np.array_equal(check_plan(np.ones((5, 7))), [[0, 0, 7, 5]])
    assert np.array_equal(check_plan(np.ones((1, 1))), [[0, 0, 1, 1]])
    assert check_plan(np.zeros((5, 7))).shape == (0, 4)
    board = np.indices((6, 7)).sum(axis=0) % 2 == 0
    assert len(check_plan(board)) == board.sum()
    ell = np.zeros((5, 6), bool)
    ell[:, 0] = True
    ell[4, :] = True
    assert np.array_equal(check_plan(ell), [[0, 0, 1, 4], [0, 4, 6, 5]])
    # a span that is interrupted for a row starts a new rectangle; two runs of one row
    gap = np.ones((4, 5), bool)
    gap[1, 2] = False
    assert np.array_equal(check_plan(gap), [[0, 0, 5, 1], [0, 1, 2, 2], [3, 1, 5, 2], [0, 2, 5, 4]])


def test_plan_on_random_grids():
    rng = np.random.default_rng(21)
    for shape in ((1, 9), (9, 1), (8, 8), (13, 17)):
        for density in (0.2, 0.5, 0.9):
            check_plan(rng.random(shape) < density)


def test_plan_refusals():
    board = np.ascontiguousarray(np.indices((4, 4)).sum(axis=0) % 2 == 0, dtype=np.uint8)
    out = np.zeros((16, 4), np.int32)
    plan = lib.load().ff_adaptive_plan_host
    assert plan(4, 4, board.ctypes.data, out.ctypes.data, 8) == 8
    assert plan(4, 4, board.ctypes.data, out.ctypes.data, 7) == -1 and "max_rects" in last_error()
    with pytest.raises(lib.FireflyError):
        lib.adaptive_plan_host(board, max_rects=3)
    assert plan(0, 4, board.ctypes.data, out.ctypes.data, 8) == -1 and "grid" in last_error()
    assert plan(4, 4, None, out.ctypes.data, 8) == -1 and "active" in last_error()
    assert plan(4, 4, board.ctypes.data, None, 8) == -1 and "out_rects4" in last_error()


# ---- the refusals of ff_render_adaptive: before the state is looked at, so they show without a device ---------------------------

def refused(ap):
    status = lib.load().ff_render_adaptive(None, None, None, C.byref(ap) if ap is not None else None, None, 0, None, 0, None, 0, None)
    return status, last_error()


def accepted_up_to_the_state(ap):
    status, text = refused(ap)
    return status == T.FF_ERR_INVALID_ARG and "state is null" in text


def test_null_adaptive_params_are_refused():
    status, text = refused(None)
    assert status == T.FF_ERR_INVALID_ARG and "ap" in text


def test_tile_is_checked():
    for tile in (0, 8, 15, 17, 48, 256, -16):
        status, text = refused(lib.adaptive_params(tile=tile))
        assert status == T.FF_ERR_INVALID_ARG and "tile" in text, tile
    for tile in T.ADAPTIVE_TILES:
        assert accepted_up_to_the_state(lib.adaptive_params(tile=tile))


def test_min_passes_is_checked():
    for value in (0, 1, 3, -2):
        status, text = refused(lib.adaptive_params(min_passes=value))
        assert status == T.FF_ERR_INVALID_ARG and "min_passes" in text, value
    assert accepted_up_to_the_state(lib.adaptive_params(min_passes=64))


def test_max_passes_is_checked():
    for lo, hi in ((4, 2), (2, 3), (2, 65535), (2, 65536), (2, 70000)):
        status, text = refused(lib.adaptive_params(min_passes=lo, max_passes=hi))
        assert status == T.FF_ERR_INVALID_ARG and "max_passes" in text, (lo, hi)
    assert accepted_up_to_the_state(lib.adaptive_params(min_passes=2, max_passes=2))
    assert accepted_up_to_the_state(lib.adaptive_params(max_passes=T.ADAPTIVE_MAX_PASSES))


def test_threshold_is_checked():
    for value in (float("nan"), float("-inf")):
        status, text = refused(lib.adaptive_params(threshold=value))
        assert status == T.FF_ERR_INVALID_ARG and "threshold" in text, value
    for value in (0.0, -1.0, 1e-30, float("inf")):
        assert accepted_up_to_the_state(lib.adaptive_params(threshold=value))


def test_flags_are_checked():
    for value in (2, 3, 0x80000000):
        status, text = refused(lib.adaptive_params(flags=value))
        assert status == T.FF_ERR_INVALID_ARG and "flags" in text, value
    assert accepted_up_to_the_state(lib.adaptive_params(flags=T.ADAPTIVE_GUARD_NEIGHBOURS))


def test_reserved_is_checked():
    status, text = refused(lib.adaptive_params(reserved=1))
    assert status == T.FF_ERR_INVALID_ARG and "reserved" in text


def test_adaptive_state_needs_a_state():
    assert lib.load().ff_adaptive_state(None, None, None, None, None, 0) == T.FF_ERR_INVALID_ARG and "state" in last_error()
    assert lib.load().ff_adaptive_tile_error(None, 1, 1, 16, 2, None, None, 0, None) == T.FF_ERR_INVALID_ARG and "state" in last_error()


# ---- the driver over the CPU oracle --------------------------------------------------------------------------------------------

def test_the_mixed_scene_is_mixed_on_the_oracle():
    """Scene and threshold are recorded in tests/adaptive_cases.py (MIX_*: open_floor_scene(area_light=True), 48 x 40, tile 16, 2 spp,
    3 bounces, passes 2 .. 8, threshold 0.0127 from the oracle's errors at n = 2)."""
    ref = oracle_drive()
    assert_mixed(ref["tile_passes"])
    first = ref["checks"][0]
    assert first["n"] == MIX_MIN and first["active_before"].all()
    assert (first["error"] == 0).any() and (first["error"] > MIX_THRESHOLD).any()
    assert ref["passes_run"] == MIX_MAX and ref["radiance"].max() > 0


def test_the_driver_of_the_restatement_on_the_oracle():
    ref = oracle_drive()
    frames = oracle_frames()
    n_t = ref["tile_passes"]
    # every tile's pixels are the mean of its own passes, its error is that of its last check, a stopped tile never resumes
    for ty in range(n_t.shape[0]):
        for tx in range(n_t.shape[1]):
            x0, y0, x1, y1 = R.tile_box(MIX_W, MIX_H, MIX_TILE, tx, ty)
            total = None
            for k in range(int(n_t[ty, tx])):
                f = frames(1234 + k, x0, y0, x1 - x0, y1 - y0)
                total = f.copy() if total is None else total + f
            assert same_bits(ref["sum"][y0:y1, x0:x1], total)
            assert same_bits(ref["radiance"][y0:y1, x0:x1], total * (F(1.0) / F(n_t[ty, tx])))
            assert (ref["passes"][y0:y1, x0:x1] == n_t[ty, tx]).all()
            stopped_at = [c["n"] for c in ref["checks"] if c["stopped"][ty, tx]]
            assert stopped_at == [int(n_t[ty, tx])] if n_t[ty, tx] < MIX_MAX else stopped_at in ([], [MIX_MAX])
    for c in ref["checks"]:
        with np.errstate(invalid="ignore"):
            assert np.array_equal(c["stopped"], c["active_before"] & (c["error"] < F(MIX_THRESHOLD)))
    # the twin reproduces the last check's errors from the sums of the tiles that were still active then
    last = ref["checks"][-1]
    twin = lib.adaptive_tile_error_host(ref["sum"], ref["sum_even"], MIX_TILE, last["n"])
    assert same_bits(twin[last["active_before"]], ref["tile_error"][last["active_before"]])
    # the rectangles: pass 0 and 1 are the whole frame
    assert ref["pixels_rendered"] == int((ref["passes"].astype(np.int64)).sum())
    assert np.array_equal(ref["rgb8"], R.to_u8(ref["radiance"]))


def test_the_guard_on_the_oracle():
    plain, guarded = oracle_drive(), oracle_drive(guard=True)
    assert (guarded["tile_passes"] >= plain["tile_passes"]).all() and (guarded["tile_passes"] > plain["tile_passes"]).any()
    grid = guarded["tile_passes"].shape
    for c in guarded["checks"]:
        with np.errstate(invalid="ignore"):
            over = c["active_before"] & ~(c["error"] < F(MIX_THRESHOLD))
        for ty, tx in zip(*np.nonzero(c["stopped"])):
            assert not over[ty, tx] and not any(over[q] for q in R.neighbours(*grid, ty, tx))
