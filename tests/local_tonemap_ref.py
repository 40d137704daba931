"""ff_local_tonemap restated in numpy float32, step by step from the text of include/firefly/ff_api.h (not from the C++): every
operation is a float32 numpy operation on whole arrays, evaluated with the parentheses the header shows, integer work on the bit
pattern through views, and np.add.at for the splat.  The kernels, the host twin and this agree bit for bit."""
import numpy as np

F = np.float32
BINS = 40
Q16_MIN, Q16_MAX = -16 * 65536, 24 * 65536 - 1
FLOOR = F(2.0 ** -16)


def luminance(rad):
    r, g, b = rad[..., 0], rad[..., 1], rad[..., 2]
    return (F(0.2126) * r + F(0.7152) * g) + F(0.0722) * b


def mapped_mask(rad, l):
    with np.errstate(invalid="ignore"):
        ok = np.isfinite(rad).all(axis=-1) & (rad >= F(0)).all(axis=-1)
        return ok & np.isfinite(l) & (l >= FLOOR)


def q16_of(l):
    """Step 1's fixed-point pseudo-log of an array of finite l >= 2^-16 (int32)."""
    bits = np.ascontiguousarray(l, dtype=F).view(np.uint32).astype(np.int64)
    e = (bits >> 23) - 127
    m = bits & 0x7FFFFF
    return np.clip(e * 65536 + (m >> 7), Q16_MIN, Q16_MAX).astype(np.int32)


def lf_of(q16):
    return q16.astype(F) * F(2.0 ** -16)


def grid_shape(h, w, s):
    return (h + s - 1) // s, (w + s - 1) // s, BINS


def splat(rad, s):
    """Step 2: (n, S) int32 [gh, gw, 40]."""
    rad = np.asarray(rad, dtype=F)
    h, w = rad.shape[:2]
    with np.errstate(all="ignore"):
        l = luminance(rad)
    ok = mapped_mask(rad, l)
    n = np.zeros(grid_shape(h, w, s), dtype=np.int32)
    S = np.zeros_like(n)
    ys, xs = np.nonzero(ok)
    q10 = q16_of(l[ys, xs]) >> 6
    z = (q10 >> 10) + 16
    np.add.at(n, (ys // s, xs // s, z), 1)
    np.add.at(S, (ys // s, xs // s, z), q10)
    return n, S


def blur_axis(v, axis):
    """Step 3 along one axis: ((v(i-1) + (2 v(i))) + v(i+1)) * 0.25, taps outside the grid 0."""
    pad = [(0, 0)] * 3
    pad[axis] = (1, 1)
    p = np.pad(v, pad).astype(F)
    idx = lambda a, b: tuple(slice(a, b) if k == axis else slice(None) for k in range(3))  # noqa: E731
    n = v.shape[axis]
    lo, c, hi = p[idx(0, n)], p[idx(1, n + 1)], p[idx(2, n + 2)]
    return ((lo + (F(2) * c)) + hi) * F(0.25)


def blur(n, S):
    """Step 3: x, then y, then z.  Arrays are [gh, gw, 40]: x is axis 1, y axis 0, z axis 2."""
    out = []
    for v in (n, S):
        v = v.astype(F)
        for axis in (1, 0, 2):
            v = blur_axis(v, axis)
        out.append(v)
    return out


def axis_taps(f, last):
    f = np.where(f < F(0), F(0), np.where(f > F(last), F(last), f)).astype(F)
    fl = np.floor(f).astype(F)
    i0 = fl.astype(np.int64)
    i1 = np.minimum(i0 + 1, last)
    return i0, i1, (f - fl).astype(F)


def lerp(a, b, t):
    return (a * (F(1) - t)) + (b * t)


def slice_grid(bn, bS, xs, ys, lf, s):
    """Step 4 for the pixels (xs, ys) with log-luminance lf: base."""
    gh, gw, _ = bn.shape
    x0, x1, tx = axis_taps(((xs.astype(F) + F(0.5)) / F(s)) - F(0.5), gw - 1)
    y0, y1, ty = axis_taps(((ys.astype(F) + F(0.5)) / F(s)) - F(0.5), gh - 1)
    z0, z1, tz = axis_taps((lf + F(16)) - F(0.5), BINS - 1)
    res = []
    for v in (bn, bS):
        v00 = lerp(v[y0, x0, z0], v[y0, x1, z0], tx)
        v10 = lerp(v[y1, x0, z0], v[y1, x1, z0], tx)
        v01 = lerp(v[y0, x0, z1], v[y0, x1, z1], tx)
        v11 = lerp(v[y1, x0, z1], v[y1, x1, z1], tx)
        v0 = lerp(v00, v10, ty)
        v1 = lerp(v01, v11, ty)
        res.append(lerp(v0, v1, tz))
    n, S = res
    with np.errstate(all="ignore"):
        return np.where(n > F(0), (S / n) * F(2.0 ** -10), lf).astype(F)


def rgb8_of(out):
    with np.errstate(all="ignore"):
        s = out * F(255)
        v = np.where(s >= F(255), F(255), s)
        v = np.where(s > F(0), v, F(0))  # (NaN -> 0)
        return v.astype(np.uint8)


def local_tonemap(rad, compression=0.5, detail=1.0, pivot=0.18, cell=32, want_gain=False):
    """The whole operator: (rgb8, radiance_out) of radiance [H,W,3]; with want_gain also g per pixel (NaN where not mapped)."""
    rad = np.ascontiguousarray(rad, dtype=F)
    out = rad.copy()
    h, w = rad.shape[:2]
    gain = np.full((h, w), np.nan, dtype=F)
    comp, det = F(compression), F(detail)
    if not (comp == F(1) and det == F(1)):
        with np.errstate(all="ignore"):
            l = luminance(rad)
        ok = mapped_mask(rad, l)
        ys, xs = np.nonzero(ok)
        if ys.size:
            n, S = splat(rad, cell)
            bn, bS = blur(n, S)
            lf = lf_of(q16_of(l[ys, xs]))
            base = slice_grid(bn, bS, xs, ys, lf, cell)
            P = lf_of(q16_of(np.array([pivot], dtype=F)))[0]
            g = ((comp - F(1)) * (base - P)) + ((det - F(1)) * (lf - base))
            g = np.where(g < F(-32), F(-32), np.where(g > F(32), F(32), g)).astype(F)
            gain[ys, xs] = g
            k = np.floor(g).astype(F)
            f = g - k
            two_k = ((k.astype(np.int64) + 127) << 23).astype(np.uint32).view(F)
            ratio = (F(1) + f) * two_k
            go = g != F(0)
            with np.errstate(over="ignore"):
                out[ys[go], xs[go]] = rad[ys[go], xs[go]] * ratio[go, None]
    res = (rgb8_of(out), out)
    return res + (gain,) if want_gain else res


def true_log_tonemap(rad, compression=0.5, detail=1.0, pivot=0.18, cell=32):
    """The same operator in float64 with true log2 / exp2 (no fixed point, no clamp of g): what the piecewise-linear pair
    approximates.  For the record (tools/local_tonemap_bench.py), not for a bit-exact comparison."""
    rad64 = np.asarray(rad, dtype=np.float64)
    out = rad64.copy()
    rad = np.ascontiguousarray(rad, dtype=F)
    with np.errstate(all="ignore"):
        l = luminance(rad)
    ok = mapped_mask(rad, l)
    ys, xs = np.nonzero(ok)
    if not ys.size:
        return out
    h, w = rad.shape[:2]
    L = np.clip(np.log2(l[ys, xs].astype(np.float64)), -16.0, 24.0 - 2.0 ** -16)
    z = np.floor(L).astype(np.int64) + 16
    n = np.zeros(grid_shape(h, w, cell), dtype=np.float64)
    S = np.zeros_like(n)
    np.add.at(n, (ys // cell, xs // cell, z), 1.0)
    np.add.at(S, (ys // cell, xs // cell, z), L)
    for axis in (1, 0, 2):
        pad = [(0, 0)] * 3
        pad[axis] = (1, 1)
        sl = lambda a, b: tuple(slice(a, b) if k == axis else slice(None) for k in range(3))  # noqa: E731
        m = n.shape[axis]
        pn, pS = np.pad(n, pad), np.pad(S, pad)
        n = (pn[sl(0, m)] + 2 * pn[sl(1, m + 1)] + pn[sl(2, m + 2)]) * 0.25
        S = (pS[sl(0, m)] + 2 * pS[sl(1, m + 1)] + pS[sl(2, m + 2)]) * 0.25
    gh, gw, _ = n.shape

    def taps(f, last):
        f = np.clip(f, 0.0, last)
        i0 = np.floor(f).astype(np.int64)
        return i0, np.minimum(i0 + 1, last), f - i0

    x0, x1, tx = taps((xs + 0.5) / cell - 0.5, gw - 1)
    y0, y1, ty = taps((ys + 0.5) / cell - 0.5, gh - 1)
    z0, z1, tz = taps(L + 16 - 0.5, BINS - 1)
    res = []
    for v in (n, S):
        a = v[y0, x0, z0] * (1 - tx) + v[y0, x1, z0] * tx
        b = v[y1, x0, z0] * (1 - tx) + v[y1, x1, z0] * tx
        c = v[y0, x0, z1] * (1 - tx) + v[y0, x1, z1] * tx
        d = v[y1, x0, z1] * (1 - tx) + v[y1, x1, z1] * tx
        res.append((a * (1 - ty) + b * ty) * (1 - tz) + (c * (1 - ty) + d * ty) * tz)
    nn, SS = res
    base = np.where(nn > 0, SS / np.where(nn > 0, nn, 1.0), L)
    g = (compression - 1.0) * (base - np.log2(pivot)) + (detail - 1.0) * (L - base)
    out[ys, xs] = rad64[ys, xs] * np.exp2(g)[:, None]
    return out
