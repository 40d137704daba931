"""A numpy float32 restatement of ff_color_grade as include/firefly/ff_api.h defines it: the primary grade, the curves on either
axis and the lattice under both interpolations, every operation a separate float32 step in the order the header writes it; and the
float64 forms of the lattice read that the accuracy tests compare against.  Test infrastructure only: written from the header's
text, not from the C++."""
import numpy as np

F = np.float32
PRIMARY, CURVES, LUT3D, TRILINEAR = 1, 2, 4, 8
AXIS_LINEAR, AXIS_LOG = 0, 1


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


def _max(a, b):
    """max(a, b) = a > b ? a : b (a NaN a gives b)."""
    return np.where(a > b, a, np.broadcast_to(b, a.shape)).astype(F)


def _min(a, b):
    return np.where(a < b, a, np.broadcast_to(b, a.shape)).astype(F)


def primary(c, matrix, offset, saturation):
    m, o, s = np.asarray(matrix, F).reshape(9), np.asarray(offset, F), F(saturation)
    r, g, b = c[..., 0], c[..., 1], c[..., 2]
    rows = []
    for i in range(3):
        t = m[3 * i] * r
        t = t + m[3 * i + 1] * g
        t = t + m[3 * i + 2] * b
        rows.append((t + o[i]).astype(F))
    lum = F(0.2126) * rows[0]
    lum = lum + F(0.7152) * rows[1]
    lum = (lum + F(0.0722) * rows[2]).astype(F)
    out = np.empty(c.shape, F)
    for i in range(3):
        d = (rows[i] - lum).astype(F)
        d = (s * d).astype(F)
        out[..., i] = lum + d
    return out


def curve_cell(x, K, axis, shift, lo, hi):
    """(k int64, t float32) of values x on the knot axis."""
    lo, hi = F(lo), F(hi)
    xc = _min(_max(x, lo), hi)
    if axis == AXIS_LOG:
        d = bits(xc).astype(np.int64) - int(F(lo).view(np.uint32))
        k = np.minimum(d >> shift, K - 2)
        rem = (d - (k << shift)).astype(F)
        t = (rem / F(1 << shift)).astype(F)
    else:
        num = (xc - lo).astype(F)
        den = F(hi - lo)
        p = (num / den).astype(F)
        p = (p * F(K - 1)).astype(F)
        k = np.minimum(np.floor(p).astype(np.int64), K - 2)
        t = (p - k.astype(F)).astype(F)
    return k, t


def curves(c, lut):
    """lut: a lib.GradeLut with curves [3, K]."""
    d, cv = lut.desc, lut.curves
    out = np.empty(c.shape, F)
    for ch in range(3):
        k, t = curve_cell(c[..., ch], d.curve_size, d.curve_axis, d.curve_shift, d.curve_lo, d.curve_hi)
        c0, c1 = cv[ch][k], cv[ch][k + 1]
        diff = (c1 - c0).astype(F)
        out[..., ch] = c0 + (t * diff).astype(F)
    return out


def lattice_cell(x, N, dmin, dmax):
    dmin, dmax = F(dmin), F(dmax)
    xc = _min(_max(x, dmin), dmax)
    u = ((xc - dmin).astype(F) / F(dmax - dmin)).astype(F)
    p = (u * F(N - 1)).astype(F)
    i = np.minimum(np.floor(p).astype(np.int64), N - 2)
    return i, (p - i.astype(F)).astype(F)


def tetra_order(fr, fg, fb):
    """The stable descending sort of (f_r, f_g, f_b): per element the axes (0 r, 1 g, 2 b) in the order A, B, C."""
    f = np.stack([fr, fg, fb], axis=-1)
    return np.argsort(-f.astype(np.float64), axis=-1, kind="stable")


def _cells(c, lut):
    d = lut.desc
    idx, fr = [], []
    for ch in range(3):
        i, f = lattice_cell(c[..., ch], d.size, d.domain_min[ch], d.domain_max[ch])
        idx.append(i)
        fr.append(f)
    return idx, fr


def _vertex(table, idx, step):
    """V at the cell (i, j, k) moved by step (dr, dg, db): table is [N, N, N, 3] indexed [b, g, r]."""
    return table[idx[2] + step[..., 2], idx[1] + step[..., 1], idx[0] + step[..., 0]]


def lattice(c, lut, trilinear, dtype=F):
    """The lattice read in `dtype` arithmetic: float32 is the restatement; float64 takes the float32 cells and fractions of the
    header exactly and evaluates only the interpolation formula in double."""
    N, table = lut.desc.size, lut.table.astype(dtype)
    idx, fr = _cells(c, lut)
    fr = [f.astype(dtype) for f in fr]
    shape = c.shape[:-1]
    zero = np.zeros(shape + (3,), np.int64)

    def at(dr, dg, db):
        return _vertex(table, idx, zero + np.array([dr, dg, db]))

    def lerp(a, b, f):
        diff = (b - a).astype(dtype)
        return (a + (f[..., None] * diff).astype(dtype)).astype(dtype)

    if trilinear:
        r00, r10 = lerp(at(0, 0, 0), at(1, 0, 0), fr[0]), lerp(at(0, 1, 0), at(1, 1, 0), fr[0])
        r01, r11 = lerp(at(0, 0, 1), at(1, 0, 1), fr[0]), lerp(at(0, 1, 1), at(1, 1, 1), fr[0])
        g0, g1 = lerp(r00, r10, fr[1]), lerp(r01, r11, fr[1])
        return lerp(g0, g1, fr[2])
    order = tetra_order(*fr)
    f = np.stack(fr, axis=-1)
    a, b, cc = (np.take_along_axis(f, order[..., n:n + 1], axis=-1)[..., 0] for n in range(3))
    eye = np.eye(3, dtype=np.int64)
    s1 = eye[order[..., 0]]
    s2 = s1 + eye[order[..., 1]]
    p0, p1, p2, p3 = at(0, 0, 0), _vertex(table, idx, s1), _vertex(table, idx, s2), at(1, 1, 1)
    out = (p0 + (a[..., None] * (p1 - p0).astype(dtype)).astype(dtype)).astype(dtype)
    out = (out + (b[..., None] * (p2 - p1).astype(dtype)).astype(dtype)).astype(dtype)
    return (out + (cc[..., None] * (p3 - p2).astype(dtype)).astype(dtype)).astype(dtype)


def color_grade(rad, p, lut=None):
    """ff_color_grade: radiance [H,W,3] float32, an FfGradeParams, a lib.GradeLut or None -> (rgb8, radiance)."""
    rad = np.ascontiguousarray(rad, F)
    flags = int(p.flags)
    with np.errstate(all="ignore"):
        c = rad.copy()
        if flags & PRIMARY:
            c = primary(c, list(p.matrix), list(p.offset), p.saturation)
        if flags & CURVES:
            c = curves(c, lut)
        if flags & LUT3D:
            c = lattice(c, lut, bool(flags & TRILINEAR))
        special = ~np.isfinite(rad).all(axis=-1)
    c = c.astype(F)
    c[special] = rad[special]
    return to_u8(c), c
