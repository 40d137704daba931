"""The tile-max skeleton of ff_motion_blur and ff_depth_of_field (csrc/ff_tile_filter.h) on the GPU, bit for bit against the numpy
references and the host twins: planted maxima and ties at the lanes, wave edges and loop trips where a reduction goes wrong
(tests/tile_filter_cases.py; test_tile_filter_host.py shows that each plant is seen in the output), the tile widths and
gather-block edges the other GPU tests leave out, degenerate guides, repeatability, and many tiles per workgroup."""
import numpy as np
import pytest

from gpupathtracer_amd import lib
import dof_cases
import dof_ref
import motion_blur_cases
import motion_blur_ref as R
import tile_filter_cases as C

pytestmark = pytest.mark.gpu

F = np.float32
K_AND_SHAPE = [(k, g) for k in C.KS for g in range(len(C.SHAPES))]
K_AND_SHAPE_IDS = [f"k{k}-{C.SHAPES[g]}" for k, g in K_AND_SHAPE]
UNVISITED_KS = [6, 10, 12, 15, 17, 23, 32, 33, 63]
BLOCK_EDGES = [(63, 5), (64, 4), (65, 3), (127, 4), (128, 5), (129, 1), (1, 129), (256, 8)]  # (w, h) around the gather's 64 x 4 pixels


def motion_all_three(tracer, rad, motion, depth, p, key=None):
    got = tracer.motion_blur(rad, motion, depth, p)
    ref = C.motion_reference(rad, motion, depth, p, key) if key else R.motion_blur(rad, motion, depth, **motion_blur_cases.params_of(p))
    motion_blur_cases.assert_same(got, ref)
    motion_blur_cases.assert_same(got, lib.motion_blur_host(rad, motion, depth, p))
    return got


def dof_all_three(tracer, rad, pos, depth, cam, p, key=None):
    got = tracer.depth_of_field(rad, (pos, depth), cam, p)
    ref = C.dof_reference(rad, pos, depth, cam, p, key) if key else dof_cases.reference(rad, pos, depth, cam, p)
    dof_cases.assert_same(got, ref)
    dof_cases.assert_same(got, lib.depth_of_field_host(rad, (pos, depth), cam, p))
    return got


def on_device_tensors(call, w, h, *images):
    """`call(pointers of the images..., rgb8 pointer, radiance_out pointer)` on device copies of host images -> (rgb8, out)."""
    import torch
    tensors = [torch.from_numpy(np.array(a)).cuda() for a in images]
    d8 = torch.zeros((h, w, 3), dtype=torch.uint8, device="cuda")
    d_out = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    call(*[t.data_ptr() for t in tensors], d8.data_ptr(), d_out.data_ptr())
    return d8.cpu().numpy(), d_out.cpu().numpy()


# ---- planted maxima ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k,group", K_AND_SHAPE, ids=K_AND_SHAPE_IDS)
def test_planted_motion_maxima_and_ties(tracer, k, group):
    """One shape of tile dominant, its winner at every plant position in turn, alone and as the first of a tie plant; one tile tie."""
    w, h = C.size_for(k)
    p = lib.motion_blur_params(shutter=C.SHUTTER, max_radius=k)
    for plan in C.plan_groups(w, h, k)[group]:
        motion_all_three(tracer, *C.planted_motion(w, h, k, plan), p, key=(k, repr(plan)))


@pytest.mark.parametrize("k,group", K_AND_SHAPE, ids=K_AND_SHAPE_IDS)
def test_planted_radii_true_maxima(tracer, k, group):
    """The same for the circle of confusion: every tile's T is a true maximum below k held by one pixel, but for one tile of
    misses and, in one plan per shape, a dominant plant at exactly k."""
    w, h = C.size_for(k)
    cam = C.camera(w, h)
    p = C.planted_dof_params(k)
    for plan in C.dof_plan_groups(w, h, k)[group]:
        dof_all_three(tracer, *C.planted_positions(w, h, k, plan, cam), cam, p, key=(k, repr(plan)))


@pytest.mark.parametrize("k,w,h", C.NARROW, ids=[f"k{k}-{w}x{h}" for k, w, h in C.NARROW])
def test_planted_images_narrower_than_a_tile(tracer, k, w, h):
    cam = C.camera(w, h)
    for plan in C.plans_for(w, h, k):
        motion_all_three(tracer, *C.planted_motion(w, h, k, plan), lib.motion_blur_params(shutter=C.SHUTTER, max_radius=k))
    for plan in C.dof_plans_for(w, h, k):
        dof_all_three(tracer, *C.planted_positions(w, h, k, plan, cam), cam, C.planted_dof_params(k))


# ---- tile widths no other GPU test runs, on the random inputs ----------------------------------------------------------------------

@pytest.mark.parametrize("k", UNVISITED_KS)
def test_unvisited_tile_widths_motion(tracer, k):
    for w, h in [(101, 67), (33, 31)]:
        rad, motion, depth = motion_blur_cases.inputs(w, h)
        for shutter in (1.0, 4.0):  # (4.0: vectors of up to 80 px, clamped to k)
            motion_all_three(tracer, rad, motion, depth, lib.motion_blur_params(shutter=shutter, max_radius=k, samples=15))


@pytest.mark.parametrize("k", UNVISITED_KS)
def test_unvisited_tile_widths_dof(tracer, k):
    for w, h in [(101, 67), (33, 31)]:
        rad, pos, depth = dof_cases.inputs(w, h)
        cam = dof_cases.camera(w, h)
        for g in (3, 1):
            dof_all_three(tracer, rad, pos, depth, cam, lib.dof_params(max_radius=k, grid=g, **dof_cases.DEFAULTS))
        # no pixel clamps: the largest radius, of the nearest point (z = 0.5: |1/2 - 2| = 1.5), is 0.9 k, so every T is a true maximum
        scale = 0.6 * k
        l, _ = dof_ref.pack(pos, depth, dof_cases.vec(cam.m_position), dof_cases.vec(cam.m_forward), 2.0, scale, k)
        assert 0.5 * k < l.max() < k
        dof_all_three(tracer, rad, pos, depth, cam, lib.dof_params(max_radius=k, grid=3, focus_distance=2.0, coc_scale=scale))


# ---- the edges of the gather's 64 x 4 workgroups -----------------------------------------------------------------------------------

@pytest.mark.parametrize("w,h", BLOCK_EDGES, ids=[f"{w}x{h}" for w, h in BLOCK_EDGES])
def test_gather_block_edges(tracer, w, h):
    rad, motion, depth = motion_blur_cases.inputs(w, h)
    d_rad, pos, d_depth = dof_cases.inputs(w, h)
    cam = dof_cases.camera(w, h)
    for k in (16, 3):
        motion_all_three(tracer, rad, motion, depth, lib.motion_blur_params(shutter=1.0, max_radius=k))
        dof_all_three(tracer, d_rad, pos, d_depth, cam, lib.dof_params(max_radius=k, **dof_cases.DEFAULTS))


# ---- degenerate guides ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", C.DEGENERATE_KS)
def test_degenerate_motion_and_depth_on_the_device(tracer, k):
    """test_tile_filter_host.py's item 3 through host buffers and through device tensors."""
    w, h = C.size_for(k)
    p = lib.motion_blur_params(shutter=C.SHUTTER, max_radius=k)
    for name, inputs, same_as, differs_from in C.degenerate_motion_cases(k):
        got = motion_all_three(tracer, *inputs, p)
        if same_as is not None:
            motion_blur_cases.assert_same(got, tracer.motion_blur(*same_as, p))
        assert (R.bits(got[1]) != R.bits(tracer.motion_blur(*differs_from, p)[1])).any(), name
        motion_blur_cases.assert_same(on_device_tensors(lambda *ptrs: tracer.motion_blur_device(w, h, *ptrs[:3], p, *ptrs[3:]), w, h, *inputs), got)


@pytest.mark.parametrize("k", C.DEGENERATE_KS)
def test_degenerate_positions_and_depth_on_the_device(tracer, k):
    w, h = C.size_for(k)
    cam = C.camera(w, h)
    for name, inputs, same_as, differs_from, overrides in C.degenerate_dof_cases(k):
        p = C.planted_dof_params(k, **overrides)
        rad, pos, depth = inputs
        got = dof_all_three(tracer, rad, pos, depth, cam, p)
        if same_as is not None:
            dof_cases.assert_same(got, tracer.depth_of_field(same_as[0], same_as[1:], cam, p))
        other = tracer.depth_of_field(differs_from[0], differs_from[1:], cam, C.planted_dof_params(k))
        assert (R.bits(got[1]) != R.bits(other[1])).any() and np.isfinite(got[1]).all(), name
        dof_cases.assert_same(on_device_tensors(lambda *ptrs: tracer.depth_of_field_device(cam, w, h, *ptrs[:3], p, *ptrs[3:]), w, h, *inputs), got)


# ---- repeatability -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [17, 64])
def test_three_runs_are_bit_identical(tracer, k):
    """The four waves' exchange through LDS and the 'whoever holds the winner writes' store: a tie plant across the wave edge
    (positions 63 and 64) in every full tile's place, three times."""
    w, h = C.size_for(k)
    cam = C.camera(w, h)
    _, _, tw, th = C.tile_box(w, h, k, 0, 0)
    plan = dict(phase=(0, 0), rot=C.positions_of(tw, th, k).index(63), tie=True)
    assert {q["index"] for q in C.motion_plants(w, h, k, plan) if q["tile"] == (0, 0)} == {63, 64}
    rad, motion, depth = C.planted_motion(w, h, k, plan)
    p = lib.motion_blur_params(shutter=C.SHUTTER, max_radius=k)
    first = motion_all_three(tracer, rad, motion, depth, p)
    d_rad, pos, d_depth = C.planted_positions(w, h, k, dict(plan, misses=1), cam)
    q = C.planted_dof_params(k)
    d_first = dof_all_three(tracer, d_rad, pos, d_depth, cam, q)
    for _ in range(2):
        motion_blur_cases.assert_same(tracer.motion_blur(rad, motion, depth, p), first)
        dof_cases.assert_same(tracer.depth_of_field(d_rad, (pos, d_depth), cam, q), d_first)


# ---- many tiles per workgroup --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", C.STRADDLE_KS)
def test_many_tiles_per_workgroup(tracer, k):
    """160 x 90 at k = 1, 2, 4: a workgroup of the lane-group kernel holds 256, 64 and 16 tiles, rows of tiles straddle workgroups,
    and tile ties lie across the seams."""
    w, h = C.STRADDLE_SIZE
    cam = C.camera(w, h)
    p = lib.motion_blur_params(shutter=C.SHUTTER, max_radius=k)
    for plan in (C.straddle_plan(k), dict(phase=(1, 1), rot=0)):
        motion_all_three(tracer, *C.planted_motion(w, h, k, plan), p, key=("straddle", k, repr(plan)))
    dof_all_three(tracer, *C.planted_positions(w, h, k, dict(phase=(1, 1), rot=0, misses=0), cam), cam, C.planted_dof_params(k))
