"""ff_local_tonemap on the GPU: bit for bit, radiance and bytes, against the host twin ff_local_tonemap_host (and through it the
numpy restatement, tests/test_local_tonemap_host.py) with host buffers, device buffers and in place, over the shapes that take each
path of the kernels - a one-pixel image, one partial cell, partial last rows and columns of cells, a column of cells one pixel
wide, several small tiles packed per workgroup - and on an empty grid, a grid of one pixel, the two-region image, the identity and
a work buffer that regrows."""
import numpy as np
import pytest

from gpupathtracer_amd import lib
import local_tonemap_ref as R
from local_tonemap_cases import GPU_SHAPES, TOL, TWO_REGION_PARAMS, assert_same, bits, hdr, params, spoiled, two_regions

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
