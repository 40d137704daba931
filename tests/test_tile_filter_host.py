"""The planted inputs of tests/tile_filter_cases.py on the host: for every tile width of KS, at one image with partial tiles on both
axes, (1) the numpy references and the host twins agree bit for bit, so the references implement the tie rules as
include/firefly/ff_api.h states them; (2) the inputs are SENSITIVE - taking a plant away, exchanging two tied pixels or two tied
tiles changes the reference's output - which is what lets test_gpu_tile_filter.py fail when the device's tile maximum T or
neighbour maximum N is wrong; (3) degenerate guides (NaN, Inf, overflowing, denormal, behind the camera) in the pixels that would
otherwise win their tiles are no motion, or a miss, bit for bit."""
import numpy as np
import pytest

from gpupathtracer_amd import lib
import dof_cases
import dof_ref
import motion_blur_cases
import motion_blur_ref as R
import tile_filter_cases as C

F = np.float32
K_AND_SHAPE = [(k, g) for k in C.KS for g in range(len(C.SHAPES))]
K_AND_SHAPE_IDS = [f"k{k}-{C.SHAPES[g]}" for k, g in K_AND_SHAPE]


def differs(a, b, mask=None):
    d = (R.bits(a[1]) != R.bits(b[1])).any(axis=-1)
    return bool((d & mask).any() if mask is not None else d.any())


def motion_twin_and_reference(rad, motion, depth, p, key=None):
    ref = C.motion_reference(rad, motion, depth, p, key) if key else R.motion_blur(rad, motion, depth, **motion_blur_cases.params_of(p))
    motion_blur_cases.assert_same(lib.motion_blur_host(rad, motion, depth, p), ref)
    return ref


def dof_twin_and_reference(rad, pos, depth, cam, p, key=None):
    ref = C.dof_reference(rad, pos, depth, cam, p, key) if key else dof_cases.reference(rad, pos, depth, cam, p)
    dof_cases.assert_same(lib.depth_of_field_host(rad, (pos, depth), cam, p), ref)
    return ref


def test_the_positions_are_the_ones_the_kernels_split_at():
    assert C.positions_of(64, 64, 64) == [0, 1, 63, 64, 255, 256, 4095]      # (tw = 64: the second row starts at the wave's edge)
    assert C.positions_of(33, 64, 64) == [0, 1, 33, 63, 64, 255, 256, 2111]  # a tile clipped at the right: another row start, another last
    assert C.positions_of(17, 17, 17) == [0, 1, 17, 63, 64, 255, 256, 288]   # one full trip and a second of 33 pixels
    assert C.positions_of(12, 12, 12) == [0, 1, 12, 63, 64, 143]             # under 256 pixels: no second trip, idle waves
    assert C.positions_of(5, 5, 5) == [0, 1, 5, 24]                          # a group of 32 lanes, 25 of them with a pixel
    assert C.positions_of(3, 5, 5) == [0, 1, 3, 14] and C.positions_of(5, 2, 5) == [0, 1, 5, 9] and C.positions_of(1, 1, 1) == [0]
    assert C.positions_of(8, 8, 8) == [0, 1, 8, 63]
    for k in C.KS:
        w, h = C.size_for(k)
        nx, ny = C.grid_of(w, h, k)
        assert nx >= 3 and ny >= 3 and (k == 1 or (w % k and h % k)) and len(C.shape_tiles(w, h, k)) == len(C.SHAPES)


@pytest.mark.parametrize("k", C.KS)
def test_every_position_of_every_shape_of_tile_wins_once(k):
    """Over a k's plans each shape of tile (full, interior, clipped right, bottom, both) is dominant with its winner at each of its
    positions, as a single plant and as the first of a tie with the next position; and there are tile ties in all three directions."""
    w, h = C.size_for(k)
    for filter_plants, plans in ((C.motion_plants, C.plans_for(w, h, k)), (C.dof_plants, C.dof_plans_for(w, h, k))):
        seen = {(q["tile"], q["index"], q["kind"]) for plan in plans for q in filter_plants(w, h, k, plan)}
        for tx, ty in C.shape_tiles(w, h, k):
            _, _, tw, th = C.tile_box(w, h, k, tx, ty)
            pos = C.positions_of(tw, th, k)
            assert {i for t, i, kind in seen if t == (tx, ty) and kind == "dominant"} == set(pos)
            if filter_plants is C.motion_plants:
                assert {i for t, i, kind in seen if t == (tx, ty) and kind == "tie_first"} == set(pos[:-1])
                assert {i for t, i, kind in seen if t == (tx, ty) and kind == "tie_second"} == set(pos[1:])
            else:
                assert any(t == (tx, ty) and kind == "clamped" for t, i, kind in seen)
        if filter_plants is C.motion_plants:
            assert len({t for t, _, kind in seen if kind == "tile_tie_first"}) >= 3


@pytest.mark.parametrize("k,group", K_AND_SHAPE, ids=K_AND_SHAPE_IDS)
def test_planted_motion_twin_parity_and_sensitivity(k, group):
    """Items 1 and 2 for ff_motion_blur.  (a) is checked for the dominant and the tied tiles of every plan, and for every tile of a
    group's first plan.  At k = 1 a tile is one pixel: there are no tie plants and (b) has nothing to check; (c) holds there as
    anywhere."""
    w, h = C.size_for(k)
    p = lib.motion_blur_params(shutter=C.SHUTTER, max_radius=k)
    base_motion, _ = C.motion_baseline(w, h, k)
    for n, plan in enumerate(C.plan_groups(w, h, k)[group]):
        rad, motion, depth = C.planted_motion(w, h, k, plan)
        plants = C.motion_plants(w, h, k, plan)
        # the plan is what it says: every tile's maximum is its plant (of a tie, the first), unclamped
        v, l, _ = R.pack(motion, depth, C.SHUTTER, k)
        assert (l < F(k)).all() and (k == 1 or l.min() > 0.5)
        T = R.tile_max(v, l, k)
        for q in plants:
            if q["kind"] != "tie_second":
                assert tuple(T[q["tile"][1], q["tile"][0], :2]) == q["v"], (plan, q)
        ref = motion_twin_and_reference(rad, motion, depth, p, key=(k, repr(plan)))
        # (a) without its plant a tile's block comes out differently
        for tile in sorted({q["tile"] for q in plants}):
            mine = [q for q in plants if q["tile"] == tile]
            if mine[0]["kind"] == "plant" and n != 0:
                continue
            without = np.array(motion)
            for q in mine:
                without[q["pixel"]] = base_motion[q["pixel"]]
            other = R.motion_blur(rad, without, depth, **motion_blur_cases.params_of(p))
            assert differs(ref, other, C.block_mask(w, h, k, *tile)), (plan, tile)
        # (b) the two pixels of a tie plant exchanged, (c) the two tiles of a tile tie exchanged
        for first, second in (("tie_first", "tie_second"), ("tile_tie_first", "tile_tie_second")):
            a, b = [q for q in plants if q["kind"] == first], [q for q in plants if q["kind"] == second]
            assert len(a) == len(b)
            for qa, qb in zip(a, b):
                qq = qa["v"][0] * qa["v"][0] + qa["v"][1] * qa["v"][1]
                assert R.bits(qq) == R.bits(qb["v"][0] * qb["v"][0] + qb["v"][1] * qb["v"][1]) and qa["v"] != qb["v"]
                swapped = np.array(motion)
                swapped[qa["pixel"]], swapped[qb["pixel"]] = motion[qb["pixel"]], motion[qa["pixel"]]
                assert differs(ref, R.motion_blur(rad, swapped, depth, **motion_blur_cases.params_of(p))), (plan, qa, qb)


@pytest.mark.parametrize("k,group", K_AND_SHAPE, ids=K_AND_SHAPE_IDS)
def test_planted_positions_twin_parity_and_sensitivity(k, group):
    """Items 1 and 2 (a) for ff_depth_of_field: its maximum has no tie rule.  (a) as for the motion."""
    w, h = C.size_for(k)
    cam = C.camera(w, h)
    p = C.planted_dof_params(k)
    base_pos, base_depth = C.dof_baseline(w, h, k)
    miss_l = F(C.dof_coc_scale(k)) * (F(1) / F(C.FOCUS))
    for n, plan in enumerate(C.dof_plan_groups(w, h, k)[group]):
        rad, pos, depth = C.planted_positions(w, h, k, plan, cam)
        plants = C.dof_plants(w, h, k, plan)
        l, _ = dof_ref.pack(pos, depth, dof_cases.vec(cam.m_position), dof_cases.vec(cam.m_forward), C.FOCUS, C.dof_coc_scale(k), k)
        T = dof_ref.tile_max(l, k)
        nx, _ = C.grid_of(w, h, k)
        assert T[plan["misses"] // nx, plan["misses"] % nx] == miss_l and 0.6 <= miss_l <= 2.0
        for q in plants:
            lq = l[q["pixel"]]
            assert T[q["tile"][1], q["tile"][0]] == lq and (lq == F(k) if q["kind"] == "clamped" else lq < F(k)), (plan, q)
            assert (l[C.block_mask(w, h, k, *q["tile"])] == lq).sum() == 1 or q["kind"] == "clamped"  # (no other pixel holds the maximum)
        ref = dof_twin_and_reference(rad, pos, depth, cam, p, key=(k, repr(plan)))
        for q in plants:
            if q["kind"] == "plant" and n != 0:
                continue
            pos2, depth2 = np.array(pos), np.array(depth)
            pos2[q["pixel"]], depth2[q["pixel"]] = base_pos[q["pixel"]], base_depth[q["pixel"]]
            assert differs(ref, dof_cases.reference(rad, pos2, depth2, cam, p), C.block_mask(w, h, k, *q["tile"])), (plan, q)


@pytest.mark.parametrize("k", C.STRADDLE_KS)
def test_tile_ties_across_workgroup_seams_are_seen(k):
    """(c) for the 160 x 90 input of the GPU test's many-tiles-per-workgroup case, and where the seams lie."""
    w, h = C.STRADDLE_SIZE
    nx, _ = C.grid_of(w, h, k)
    plan = C.straddle_plan(k)
    per = {1: 256, 2: 64, 4: 16}[k]
    (a, b), (c, d) = [[ty * nx + tx for tx, ty in pair] for pair in plan["tile_ties"]]
    assert b == a + 1 and a // per != b // per and a // nx == b // nx  # side by side in one row of tiles, in two workgroups
    assert d == c + nx and c // per != d // per
    p = lib.motion_blur_params(shutter=C.SHUTTER, max_radius=k)
    rad, motion, depth = C.planted_motion(w, h, k, plan)
    ref = motion_twin_and_reference(rad, motion, depth, p, key=("straddle", k, repr(plan)))
    plants = C.motion_plants(w, h, k, plan)
    firsts, seconds = ([q for q in plants if q["kind"] == kind] for kind in ("tile_tie_first", "tile_tie_second"))
    assert len(firsts) == len(seconds) == 2
    for qa, qb in zip(firsts, seconds):
        swapped = np.array(motion)
        swapped[qa["pixel"]], swapped[qb["pixel"]] = motion[qb["pixel"]], motion[qa["pixel"]]
        assert differs(ref, R.motion_blur(rad, swapped, depth, **motion_blur_cases.params_of(p))), (qa, qb)


@pytest.mark.parametrize("k", C.DEGENERATE_KS)
def test_degenerate_motion_and_depth_never_win_a_tile(k):
    """Item 3 for ff_motion_blur.  A depth of 1e-45 is finite and > 0: by ff_api.h it is a hit, the nearest there is, so it is
    compared between reference and twin only (and seen to differ from a miss)."""
    for name, (rad, motion, depth), same_as, differs_from in C.degenerate_motion_cases(k):
        p = lib.motion_blur_params(shutter=C.SHUTTER, max_radius=k)
        got = motion_twin_and_reference(rad, motion, depth, p)
        if same_as is not None:
            motion_blur_cases.assert_same(got, motion_twin_and_reference(*same_as, p))
        assert differs(got, motion_twin_and_reference(*differs_from, p)), name


@pytest.mark.parametrize("k", C.DEGENERATE_KS)
def test_degenerate_positions_and_depth_are_misses(k):
    """Item 3 for ff_depth_of_field.  Two values stay hits by ff_api.h and are held to that: a point 1e30 ahead (z is finite; its l
    is a miss's, coc_scale |fi - 1e-30| = coc_scale fi, its zk is not) and a depth of 1e-45 (finite and > 0; l comes from the
    position alone, so the output is the unspoiled one)."""
    w, h = C.size_for(k)
    cam = C.camera(w, h)
    for name, (rad, pos, depth), same_as, differs_from, overrides in C.degenerate_dof_cases(k):
        p = C.planted_dof_params(k, **overrides)
        got = dof_twin_and_reference(rad, pos, depth, cam, p)
        if same_as is not None:
            dof_cases.assert_same(got, dof_twin_and_reference(*same_as, cam, p))
        assert differs(got, dof_twin_and_reference(*differs_from, cam, C.planted_dof_params(k))), name
        assert np.isfinite(got[1]).all()
    # the point 1e30 ahead: a hit with a miss's radius
    name, (rad, pos, depth), _, _, _ = [c for c in C.degenerate_dof_cases(k) if c[0] == "position 1e30 ahead"][0]
    l, zk = dof_ref.pack(pos, depth, dof_cases.vec(cam.m_position), dof_cases.vec(cam.m_forward), C.FOCUS, C.dof_coc_scale(k), k)
    assert ((zk == F(1e30)) & (l == F(C.dof_coc_scale(k)) * (F(1) / F(C.FOCUS)))).sum() == 1
