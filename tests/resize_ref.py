"""A numpy restatement of ff_resize as include/firefly/ff_api.h defines it: the per-axis table in float64, every formula left to right
as the header writes it, and the two passes in float32 over tables that are passed in (the library's own, where a test wants bit
parity whatever its libm's sin does).  Every float32 operation is its own numpy operation (no fused multiply-add); min and max are
np.where as the header defines them, taken tap after tap."""
import numpy as np

F = np.float32
BOX, TRIANGLE, MITCHELL, LANCZOS3 = 0, 1, 2, 3
FILTERS = (BOX, TRIANGLE, MITCHELL, LANCZOS3)
ANTI_RING = 1            # FF_RESIZE_ANTI_RING
RADIUS = {BOX: 0.5, TRIANGLE: 1.0, MITCHELL: 2.0, LANCZOS3: 3.0}
MAX_RATIO, MAX_TAPS = 16, 96


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def to_u8(v):
    """trunc(clamp(v * 255)); NaN -> 0."""
    with np.errstate(invalid="ignore", over="ignore"):
        s = np.asarray(v, F) * F(255.0)
        out = np.zeros(s.shape, np.uint8)
        mid = (s > 0) & (s < F(255.0))
        out[mid] = s[mid].astype(np.uint8)
        out[s >= F(255.0)] = 255
    return out


def kernel(filter, t):
    """k(t) for a float64 array t."""
    t = np.asarray(t, np.float64)
    a = np.abs(t)
    if filter == BOX:
        return np.where((-0.5 <= t) & (t < 0.5), 1.0, 0.0)
    if filter == TRIANGLE:
        return np.where(a < 1.0, 1.0 - a, 0.0)
    if filter == MITCHELL:
        B = C = 1.0 / 3.0
        near = ((12.0 - 9.0 * B - 6.0 * C) * a * a * a + (-18.0 + 12.0 * B + 6.0 * C) * a * a + (6.0 - 2.0 * B)) / 6.0
        far = ((-B - 6.0 * C) * a * a * a + (6.0 * B + 30.0 * C) * a * a + (-12.0 * B - 48.0 * C) * a + (8.0 * B + 24.0 * C)) / 6.0
        return np.where(a < 1.0, near, np.where(a < 2.0, far, 0.0))
    assert filter == LANCZOS3
    pi = np.pi
    with np.errstate(invalid="ignore", divide="ignore"):
        lobe = 3.0 * np.sin(pi * t) * np.sin(pi * t / 3.0) / (pi * pi * t * t)
    return np.where(a >= 3.0, 0.0, np.where(t == 0.0, 1.0, np.where(t == np.floor(t), 0.0, lobe)))


def taps(n, N, filter):
    s = float(n) / float(N)
    f = max(s, 1.0)
    return int(np.ceil(2.0 * (RADIUS[filter] * f)))


def table(n, N, filter, full=False):
    """(first int32 [N], weights float32 [N, T]) of an axis of n input and N output samples.  full: also (k, S, c, r, f) in
    float64."""
    s = float(n) / float(N)
    f = max(s, 1.0)
    r = RADIUS[filter] * f
    T = int(np.ceil(2.0 * r))
    X = np.arange(N, dtype=np.float64)
    c = (X + 0.5) * s - 0.5
    first = np.ceil(c - r).astype(np.int64)
    k = np.empty((N, T), np.float64)
    S = np.zeros(N, np.float64)
    for j in range(T):
        k[:, j] = kernel(filter, ((first + j).astype(np.float64) - c) / f)
        S = S + k[:, j]
    w = (k / S[:, None]).astype(F)
    if full:
        return first.astype(np.int32), w, (k, S, c, r, f)
    return first.astype(np.int32), w


def fmin(a, b):
    """min(a, b) = b < a ? b : a"""
    return np.where(b < a, b, a).astype(F)


def fmax(a, b):
    """max(a, b) = a < b ? b : a"""
    return np.where(a < b, b, a).astype(F)


def resample(img, first, weights, ring, axis):
    """One pass over `axis` (0: rows are resampled, i.e. the vertical pass; 1: the horizontal pass) of img [H,W,3] float32."""
    img = np.asarray(img, F)
    n = img.shape[axis]
    N, T = weights.shape
    shape = list(img.shape)
    shape[axis] = N
    acc = np.zeros(shape, F)
    lo = np.full(shape, np.inf, F)
    hi = np.full(shape, -np.inf, F)
    wshape = [1, 1, 1]
    wshape[axis] = N
    with np.errstate(invalid="ignore", over="ignore"):
        for j in range(T):
            idx = np.clip(first.astype(np.int64) + j, 0, n - 1)
            v = np.take(img, idx, axis=axis)
            v = np.where(np.isfinite(v), v, F(0.0)).astype(F)
            w = weights[:, j].astype(F).reshape(wshape)
            acc = (acc + (w * v).astype(F)).astype(F)
            if ring:
                named = np.broadcast_to(w != 0, v.shape)
                lo = np.where(named, fmin(lo, v), lo).astype(F)
                hi = np.where(named, fmax(hi, v), hi).astype(F)
        if ring:
            acc = fmin(fmax(acc, lo), hi)
    return acc


def resize(img, table_x, table_y, flags):
    """The two passes, the horizontal one first, with tables (first, weights) per axis -> (rgb8, radiance)."""
    ring = bool(flags & ANTI_RING)
    mid = resample(img, table_x[0], table_x[1], ring, axis=1)
    out = resample(mid, table_y[0], table_y[1], ring, axis=0)
    return to_u8(out), out
