"""What tests/test_yuv_host.py and tests/test_gpu_yuv.py share: the parameter sets, the input images and the comparison."""
import itertools

import numpy as np

from gpupathtracer_amd import lib
from gpupathtracer_amd import types as T
import yuv_ref as R

F = np.float32

TRANSFERS = (T.YUV_TRANSFER_BT709, T.YUV_TRANSFER_SRGB, T.YUV_TRANSFER_PQ)
MATRICES = (T.YUV_MATRIX_BT709, T.YUV_MATRIX_BT2020)
RANGES = (T.YUV_RANGE_LIMITED, T.YUV_RANGE_FULL)
DEPTHS = (8, 10)
SITINGS = (T.YUV_SITING_CENTER, T.YUV_SITING_LEFT)
ALL_COMBINATIONS = list(itertools.product(TRANSFERS, MATRICES, RANGES, DEPTHS, SITINGS))

HOST_SIZES = [(1, 1), (2, 2), (3, 3), (5, 2), (7, 5), (66, 19)]
# around the lane's 4 x 2 block and the kernel's 64 x 32 tile (and every smaller power-of-two edge)
GPU_SIZES = [(1, 1), (2, 2), (3, 3), (5, 2), (7, 5), (64, 16), (65, 17), (67, 19), (130, 35)]
SEAM_SIZE = (130, 35)
SEAM_COLUMNS, SEAM_ROWS = (63, 64, 65, 127, 128), (15, 16, 17)


def params(transfer=T.YUV_TRANSFER_BT709, matrix=T.YUV_MATRIX_BT709, range_=T.YUV_RANGE_LIMITED, depth=8, siting=T.YUV_SITING_LEFT, **more):
    return lib.yuv_params(transfer=transfer, matrix=matrix, range=range_, depth=depth, siting=siting, **more)


def gpu_param_sets():
    return {
        "nv12-bt709-limited-left": params(),
        "p010-pq-bt2020-limited-left": params(T.YUV_TRANSFER_PQ, T.YUV_MATRIX_BT2020, T.YUV_RANGE_LIMITED, 10, T.YUV_SITING_LEFT),
        "nv12-srgb-full-center": params(T.YUV_TRANSFER_SRGB, T.YUV_MATRIX_BT709, T.YUV_RANGE_FULL, 8, T.YUV_SITING_CENTER),
    }


def name_of(combo):
    t, m, r, d, s = combo
    return f"{('bt709', 'srgb', 'pq')[t]}-{('m709', 'm2020')[m]}-{('limited', 'full')[r]}-{d}-{('center', 'left')[s]}"


def inputs(w, h, transfer=T.YUV_TRANSFER_BT709, seed=0):
    """A w x h image whose values span 0 .. 60: a third in 0 .. 1, a third up to 60 (log-uniform), and a third exact knots of the
    transfer and the floats on either side of one (for PQ divided by the default scale, so that they land near knots after step 3)."""
    rng = np.random.default_rng(1000 * w + h + 17 * seed + 7)
    n = w * h * 3
    low = rng.random(n).astype(F)
    high = np.exp(rng.uniform(np.log(1e-4), np.log(60.0), n)).astype(F)
    K = R.knots(transfer)
    k = K[rng.integers(0, R.CELLS + 1, n)]
    side = rng.integers(-1, 2, n)
    k = np.where(side < 0, np.nextafter(k, F(-1)), np.where(side > 0, np.nextafter(k, F(2)), k)).astype(F)
    if transfer == T.YUV_TRANSFER_PQ:
        k = (k / (F(203) / F(10000))).astype(F)
    pick = rng.integers(0, 3, n)
    img = np.where(pick == 0, low, np.where(pick == 1, high, k)).astype(F)
    img = np.maximum(img, F(0))
    return np.ascontiguousarray(img.reshape(h, w, 3))


def assert_same(got, want, what=""):
    """Two (luma, chroma) pairs agree byte for byte."""
    for name, g, e in zip(("luma", "chroma"), got, want):
        g, e = np.asarray(g), np.asarray(e)
        assert g.shape == e.shape and g.dtype.itemsize == e.dtype.itemsize, (what, name, g.shape, e.shape, g.dtype, e.dtype)
        g = g.view(e.dtype) if g.dtype != e.dtype else g
        bad = np.argwhere(g != e)
        assert bad.size == 0, f"{what} {name}: {len(bad)} samples differ, first at {bad[0].tolist()}: {g[tuple(bad[0])]} != {e[tuple(bad[0])]}"


def unshift(planes, depth):
    """(Y [H,W], Cb, Cr [ch,cw]) integer codes of a (luma, chroma) pair."""
    luma, chroma = (np.asarray(a).astype(np.int64) >> (0 if depth == 8 else 6) for a in planes)
    return luma, chroma[..., 0], chroma[..., 1]
