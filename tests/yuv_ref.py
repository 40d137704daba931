"""ff_encode_yuv restated in numpy float32 (include/firefly/ff_api.h, steps 1 to 8), written from the header alone: every operation is
one IEEE float32 operation in the header's order, so the library's kernel and host twin must agree with it bit for bit.  The knots
are evaluated here in Python float64 (the same libm pow the library calls) and rounded to float32.  true_codes() is the float64
"true form" with the real pow OETFs and round-half-up that the deviation test compares against."""
import functools
import math

import numpy as np

F = np.float32
BT709, SRGB, PQ = 0, 1, 2
M_BT709, M_BT2020 = 0, 1
LIMITED, FULL = 0, 1
CENTER, LEFT = 0, 1
CELLS = 4096

PQ_M1, PQ_M2 = 2610.0 / 16384.0, 2523.0 / 4096.0 * 128.0
PQ_C1, PQ_C2, PQ_C3 = 3424.0 / 4096.0, 2413.0 / 4096.0 * 32.0, 2392.0 / 4096.0 * 32.0
GAMUT = ((0.6274, 0.3293, 0.0433), (0.0691, 0.9195, 0.0114), (0.0164, 0.0880, 0.8956))
COEFFS = {M_BT709: (0.2126, 0.7152, 0.0722, 1.8556, 1.5748), M_BT2020: (0.2627, 0.6780, 0.0593, 1.8814, 1.4746)}


def eotf(transfer, s):
    """Step 4's EOTF of one Python float in [0, 1]."""
    if transfer == SRGB:
        return s / 12.92 if s <= 0.04045 else math.pow((s + 0.055) / 1.055, 2.4)
    if transfer == BT709:
        return s / 4.5 if s < 0.081 else max(math.pow((s + 0.099) / 1.099, 1.0 / 0.45), 0.081 / 4.5)
    p = math.pow(s, 1.0 / PQ_M2)
    return math.pow(max(p - PQ_C1, 0.0) / (PQ_C2 - PQ_C3 * p), 1.0 / PQ_M1)


@functools.lru_cache(maxsize=None)
def _knots(transfer):
    k = np.array([eotf(transfer, j / CELLS) for j in range(CELLS + 1)], dtype=np.float64).astype(F)
    k.setflags(write=False)
    return k


def knots(transfer):
    return _knots(int(transfer))


def transfer_f32(K, v):
    """Step 4's evaluation for a float32 array 0 <= v <= 1."""
    j = np.zeros(v.shape, np.int64)
    step = CELLS // 2
    while step >= 1:
        j = np.where(K[j + step] <= v, j + step, j)
        step >>= 1
    k0, k1 = K[j], K[j + 1]
    e = (j.astype(F) + (v - k0) / (k1 - k0)) * F(1.0 / CELLS)
    return np.where(v >= F(1), F(1), e).astype(F)


def _taps(c, xs, ys):
    h, w = c.shape
    return c[np.clip(ys, 0, h - 1)[:, None], np.clip(xs, 0, w - 1)[None, :]]


def chroma_filter(c, siting, half=0.5, quarter=0.25):
    """Step 6 for one plane; the dtype of c decides the arithmetic."""
    h, w = c.shape
    t = c.dtype.type
    X, Y = np.arange((w + 1) // 2), np.arange((h + 1) // 2)
    if siting == CENTER:
        return ((_taps(c, 2 * X, 2 * Y) + _taps(c, 2 * X + 1, 2 * Y)) + (_taps(c, 2 * X, 2 * Y + 1) + _taps(c, 2 * X + 1, 2 * Y + 1))) * t(quarter)
    def hrow(ys):
        return (_taps(c, 2 * X - 1, ys) * t(quarter) + _taps(c, 2 * X, ys) * t(half)) + _taps(c, 2 * X + 1, ys) * t(quarter)
    return (hrow(2 * Y) + hrow(2 * Y + 1)) * t(half)


def quantise(y, cb, cr, full, depth, t=F):
    """Step 7 in the arithmetic of type t: integer codes."""
    s, m, mid = t(2 ** (depth - 8)), t(2 ** depth - 1), t(2 ** (depth - 1))
    if full:
        Y = np.floor(y * m + t(0.5))
        C = [np.clip(np.floor((c * m + mid) + t(0.5)), t(0), m) for c in (cb, cr)]
    else:
        Y = np.floor((t(219) * y + t(16)) * s + t(0.5))
        C = [np.clip(np.floor((t(224) * c + t(128)) * s + t(0.5)), t(16) * s, t(240) * s) for c in (cb, cr)]
    return Y.astype(np.int64), C[0].astype(np.int64), C[1].astype(np.int64)


def pixel_values(linear, p):
    """Steps 1 to 5 in float32: (y, cb, cr) planes, unquantised."""
    c = np.asarray(linear, dtype=F)
    with np.errstate(invalid="ignore"):
        c = np.where(c > F(0), c, F(0)).astype(F)
    c = np.minimum(c, F(65536))
    r, g, b = c[..., 0], c[..., 1], c[..., 2]
    if p.matrix == M_BT2020:
        r, g, b = [(F(m[0]) * r + F(m[1]) * g) + F(m[2]) * b for m in GAMUT]
    if p.transfer == PQ:
        scale = F(p.reference_white_nits) / F(10000)
        r, g, b = r * scale, g * scale, b * scale
    K = knots(p.transfer)
    r, g, b = [transfer_f32(K, np.minimum(v, F(1))) for v in (r, g, b)]
    kr, kg, kb, dcb, dcr = [F(v) for v in COEFFS[int(p.matrix)]]
    y = (kr * r + kg * g) + kb * b
    return y, (b - y) / dcb, (r - y) / dcr


def codes(linear, p):
    """Steps 1 to 7: integer code planes (Y [H,W], Cb and Cr [ceil(H/2),ceil(W/2)])."""
    y, cb, cr = pixel_values(linear, p)
    return quantise(y, chroma_filter(cb, int(p.siting)), chroma_filter(cr, int(p.siting)), p.range == FULL, int(p.depth))


def encode(linear, p):
    """ff_encode_yuv: (luma [H,W], chroma [ceil(H/2),ceil(W/2),2]); uint8 at depth 8, uint16 (code << 6) at depth 10."""
    Y, Cb, Cr = codes(linear, p)
    dtype, shift = (np.uint8, 0) if int(p.depth) == 8 else (np.uint16, 6)
    return (Y << shift).astype(dtype), (np.stack([Cb, Cr], axis=-1) << shift).astype(dtype)


def oetf_true(transfer, v):
    """The real OETF (the exact inverse of eotf) of a float64 array in [0, 1]."""
    v = np.asarray(v, dtype=np.float64)
    if transfer == SRGB:
        return np.where(v <= 0.04045 / 12.92, v * 12.92, 1.055 * np.power(v, 1.0 / 2.4) - 0.055)
    if transfer == BT709:
        return np.where(v < 0.081 / 4.5, v * 4.5, 1.099 * np.power(v, 0.45) - 0.099)
    q = np.power(v, PQ_M1)
    return np.power((PQ_C1 + PQ_C2 * q) / (1.0 + PQ_C3 * q), PQ_M2)


def true_codes(linear, p):
    """The float64 true form: the same steps with the real pow OETFs, the matrices in double and round-half-up."""
    c = np.asarray(linear, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        c = np.where(c > 0, c, 0.0)
    c = np.minimum(c, 65536.0)
    r, g, b = c[..., 0], c[..., 1], c[..., 2]
    if p.matrix == M_BT2020:
        r, g, b = [(m[0] * r + m[1] * g) + m[2] * b for m in GAMUT]
    if p.transfer == PQ:
        scale = float(p.reference_white_nits) / 10000.0
        r, g, b = r * scale, g * scale, b * scale
    r, g, b = [oetf_true(int(p.transfer), np.minimum(v, 1.0)) for v in (r, g, b)]
    kr, kg, kb, dcb, dcr = COEFFS[int(p.matrix)]
    y = (kr * r + kg * g) + kb * b
    cb, cr = (b - y) / dcb, (r - y) / dcr
    return quantise(y, chroma_filter(cb, int(p.siting)), chroma_filter(cr, int(p.siting)), p.range == FULL, int(p.depth), t=np.float64)
