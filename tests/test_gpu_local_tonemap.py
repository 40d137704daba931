"""ff_local_tonemap on the GPU: bit for bit, radiance and bytes, against the host twin ff_local_tonemap_host (and through it the
numpy restatement, tests/test_local_tonemap_host.py) with host buffers, device buffers and in place, over the shapes that take each
path of the kernels - a one-pixel image, one partial cell, partial last rows and columns of cells, a column of cells one pixel
wide, several small tiles packed per workgroup, every cell size over several cell rows and columns with partial last cells - and
on an empty grid, a grid of one pixel, the two-region image, cell sums beyond float precision, a checker that leaves the splat no
run to merge, cells emptied between two calls on one state, the identity and a work buffer that regrows."""
import numpy as np
import pytest

from gpupathtracer_amd import lib
import local_tonemap_ref as R
from local_tonemap_cases import (CELLS, EXTREME_STOPS, GPU_SHAPES, TOL, TWO_REGION_PARAMS, assert_same, bin_checker, bits, extreme, hdr, longest_run, params,
                                 spoiled, stale_bases, stale_pair, two_regions)

pytestmark = pytest.mark.gpu

F = np.float32
SHAPES = [(w, h, cell) for w, h, cells in GPU_SHAPES for cell in cells]


def check_every_buffer_kind(tracer, rad, p):
    """Host buffers, device buffers, in place on the device and in place through the staging: all the twin's bits."""
    import torch
    want = lib.local_tonemap_host(rad, p)
    assert_same(tracer.local_tonemap(rad, p), want)
    assert_same(tracer.local_tonemap(rad, p, in_place=True), want)
    dev = torch.from_numpy(np.array(rad)).cuda()
    rgb8, out = tracer.local_tonemap(dev, p)
    assert_same((rgb8.cpu().numpy(), out.cpu().numpy()), want)
    assert np.array_equal(bits(dev.cpu().numpy()), bits(rad))  # (the input is left alone)
    rgb8, out = tracer.local_tonemap(dev, p, in_place=True)
    assert out.data_ptr() == dev.data_ptr()
    assert_same((rgb8.cpu().numpy(), dev.cpu().numpy()), want)
    return want


@pytest.mark.parametrize("w,h,cell", SHAPES, ids=[f"{w}x{h}-cell{cell or 'default'}" for w, h, cell in SHAPES])
def test_kernels_match_the_twin_bit_for_bit(tracer, w, h, cell):
    rad = spoiled(w, h)[0] if w * h > 64 else hdr(w, h)
    changed = 0
    for compression, detail in [(0.5, 1.0), (0.0, 2.0), (1.0, 0.0)]:
        p = params(compression=compression, detail=detail) if cell is None else params(compression=compression, detail=detail, cell=cell)
        out = check_every_buffer_kind(tracer, rad, p)[1]
        changed += int((bits(out) != bits(rad)).sum())
    assert changed


@pytest.mark.parametrize("cell", CELLS)
@pytest.mark.parametrize("stop", list(EXTREME_STOPS))
def test_long_runs_and_sums_beyond_float_precision(tracer, stop, cell):
    """Flat and two-level 128 x 128 images in the top stop and in the bottom mapped stop: a splat thread of cell 64 merges its 16
    pixels into one add, a full cell of 64 sums q10 beyond +-2^24 and the x blur's (float)int rounds it (asserted here for cell 64
    through the grid twin; tests/test_local_tonemap_host.py holds the twin against the restatement on the same images)."""
    for two_level in (False, True):
        rad = extreme(stop, two_level)
        _, S = lib.local_tonemap_grid_host(rad, params(cell=64))
        assert (np.abs(S.astype(np.int64)).max(axis=2) > 2 ** 24).all()
        if two_level:
            assert (S.astype(F).astype(np.int64) != S).any()
        assert longest_run(rad, 64) == 16
        for compression, detail in [(0.5, 1.0), (0.0, 2.0)]:
            out = check_every_buffer_kind(tracer, rad, params(cell=cell, compression=compression, detail=detail))[1]
            assert (bits(out) != bits(rad)).any()


@pytest.mark.parametrize("cell", CELLS)
def test_checker_of_two_bins(tracer, cell):
    """A one-pixel checker of two adjacent bins, plain and shifted every 256 / cell rows, so that no run of a splat thread of cell 32
    or 64 is longer than one pixel: every add is a thread's own."""
    rows = 256 // cell if cell * cell > 256 else 0
    assert longest_run(bin_checker(rows), cell) == 1
    for rad in {0: bin_checker(), rows: bin_checker(rows)}.values():
        check_every_buffer_kind(tracer, rad, params(cell=cell, detail=2.0))


@pytest.mark.parametrize("cell", CELLS)
def test_emptied_cells_are_written_again(tracer, cell):
    """The splat writes empty cells, so the grid is never cleared: on one state a fully mapped 130 x 70 image, then the same size
    with chosen cells wholly unmapped (for cell 8 one tile of the four in a workgroup, and the last, partial workgroup) - host
    buffers, then device buffers.  The second result is the twin's bit for bit; that a stale cell would change it is asserted
    through the grid twin: the cells are empty, and a mapped pixel next to each gets another base than the first image's cell
    would give it."""
    import torch
    first, second, cells = stale_pair(cell)
    p = params(cell=cell, detail=2.0)
    n1, _ = lib.local_tonemap_grid_host(first, p)
    n2, _ = lib.local_tonemap_grid_host(second, p)
    for cy, cx in cells:
        assert n1[cy, cx].any() and not n2[cy, cx].any()
    for at, true, stale in stale_bases(cell):
        assert true != stale, (at, true, stale)
    want1, want2 = lib.local_tonemap_host(first, p), lib.local_tonemap_host(second, p)
    assert (bits(want1[1]) != bits(want2[1]))[second[..., 0] >= 0].any()
    assert_same(tracer.local_tonemap(first, p), want1)
    assert_same(tracer.local_tonemap(second, p), want2)
    d_first, d_second = (torch.from_numpy(np.array(a)).cuda() for a in (first, second))
    rgb8, out = tracer.local_tonemap(d_first, p)
    assert_same((rgb8.cpu().numpy(), out.cpu().numpy()), want1)
    rgb8, out = tracer.local_tonemap(d_second, p)
    assert_same((rgb8.cpu().numpy(), out.cpu().numpy()), want2)


def test_only_one_output_at_a_time(tracer):
    rad = hdr(33, 17)
    p = params(cell=16)
    want = lib.local_tonemap_host(rad, p)
    rgb8, none = tracer.local_tonemap(rad, p, want_out=False)
    assert none is None and np.array_equal(rgb8, want[0])
    none, out = tracer.local_tonemap(rad, p, want_rgb8=False)
    assert none is None and np.array_equal(bits(out), bits(want[1]))


def test_all_unmapped_image_gives_an_empty_grid_and_a_copy(tracer):
    rad = np.zeros((33, 65, 3), F)
    rad[::2] = (-1.0, 2.0, 3.0)
    rad[1::4, ::3] = (np.nan, 1.0, np.inf)
    rad[3::4, 1::3] = 2.0 ** -18
    n, _ = lib.local_tonemap_grid_host(rad, params(cell=8))
    assert not n.any()
    for cell in (8, 32):
        rgb8, out = check_every_buffer_kind(tracer, rad, params(cell=cell, detail=2.0))
        assert np.array_equal(bits(out), bits(rad)) and np.array_equal(rgb8, R.rgb8_of(rad))


def test_one_mapped_pixel(tracer):
    """One mapped pixel among unmapped ones: its base is its own log-luminance (S / n = q10 whatever weight the blur left), so
    the detail term vanishes and the gain is the compression's alone."""
    rad = np.zeros((33, 65, 3), F)
    rad[:, ::2] = (np.nan, 0.0, 0.0)
    rad[20, 41] = 8.0  # Lf = 3; pivot 1: g = -0.5 * 3 = -1.5 -> k = -2, f = 0.5, ratio 0.375
    for cell in (8, 16, 64):
        n, _ = lib.local_tonemap_grid_host(rad, params(cell=cell))
        assert int(n.sum()) == 1
        rgb8, out = check_every_buffer_kind(tracer, rad, params(cell=cell, pivot=1.0, detail=3.0))
        assert np.abs(out[20, 41] / 3.0 - 1.0).max() <= TOL
        keep = np.ones(rad.shape[:2], bool)
        keep[20, 41] = False
        assert np.array_equal(bits(out)[keep], bits(rad)[keep])


def test_two_regions_on_the_device(tracer):
    for checker in (False, True):
        rad = two_regions(checker)
        _, out = check_every_buffer_kind(tracer, rad, params(**TWO_REGION_PARAMS))
        assert np.abs(out[:, :64].astype(np.float64) / 0.375 - 1.0).max() <= TOL
        if not checker:
            assert np.abs(out[:, 64:].astype(np.float64) / 6.0 - 1.0).max() <= TOL


def test_identity_on_the_device(tracer):
    rad = np.array(spoiled(65, 33)[0])
    rad[0, 0] = np.array([0x7FC01234, 0xFF800000, 0x80000000], np.uint32).view(F)  # a NaN with a payload, -Inf, -0
    for cell in (8, 64):
        rgb8, out = check_every_buffer_kind(tracer, rad, params(compression=1.0, detail=1.0, cell=cell))
        assert np.array_equal(bits(out), bits(rad)) and np.array_equal(rgb8, R.rgb8_of(rad))


def test_work_buffer_regrows_between_calls_of_different_sizes(tracer):
    """A small call, a larger one (more cells and more staging), the small one again - on one state, and on a fresh one so that
    the first call allocates."""
    small, big = hdr(7, 5), spoiled(130, 70)[0]
    with lib.Tracer(0) as fresh:
        for t in (fresh, tracer):
            for rad, cell in [(small, 64), (big, 8), (small, 8), (big, 16)]:
                p = params(cell=cell, detail=2.0)
                assert_same(t.local_tonemap(rad, p), lib.local_tonemap_host(rad, p))
