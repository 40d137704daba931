"""ff_lens restated in numpy float32 from include/firefly/ff_api.h: steps 1 to 5 per output pixel and channel, vectorised over the
image, every expression parenthesised as the header writes it.  The two tables are consumed as ff_lens_tables returns them
(tests/test_lens_host.py checks them against the closed form in float64, which `model_tables` below states)."""
import numpy as np

F = np.float32
KNOTS = 1024
UNDISTORT, DISTORT = 0, 1
BILINEAR, CATMULL_ROM = 0, 1
BLACK, CLAMP = 0, 1
ANTI_RING = 1


def bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


def to_u8(v):
    """The project's 8-bit rule: trunc(clamp(v * 255)), NaN -> 0."""
    with np.errstate(invalid="ignore", over="ignore"):
        s = np.asarray(v, F) * F(255.0)
        out = np.where(s > 0, np.where(s >= F(255.0), F(255.0), s), F(0.0))
    return out.astype(np.uint8)


def constants(w, h, p, r2_max):
    """(cx, cy, inv_d2, knot_scale) as the kernel gets them."""
    cx = F(0.5) * F(w) + F(p.center_x)
    cy = F(0.5) * F(h) + F(p.center_y)
    d2 = 0.25 * (float(w) * float(w) + float(h) * float(h))
    return cx, cy, F(1.0 / d2), F(float(KNOTS) / r2_max)


def radial(w, h, p, tables, px, py):
    """Step 1 at the float32 positions px, py -> dx, dy, e, gain."""
    e_t, g_t, r2_max = tables
    cx, cy, inv_d2, knot_scale = constants(w, h, p, r2_max)
    dx = px - cx
    dy = py - cy
    r2 = ((dx * dx) + (dy * dy)) * inv_d2
    u = r2 * knot_scale
    u = np.where(u < F(KNOTS), u, F(KNOTS))
    i = np.clip(np.floor(u).astype(np.int64), 0, KNOTS - 1)
    t = u - i.astype(F)
    e = e_t[i] + t * (e_t[i + 1] - e_t[i])
    g = g_t[i] + t * (g_t[i + 1] - g_t[i])
    return dx, dy, e, g


def source(px, py, dx, dy, e, q):
    """Step 2 for the channel of magnification q."""
    q = F(q)
    ec = (e + q) + (e * q)
    return px + (dx * ec), py + (dy * ec)


def map_positions(w, h, p, tables, xy, channel=1):
    """ff_lens_map_host restated: float32 [n,2] -> float32 [n,2]."""
    xy = np.asarray(xy, F)
    px, py = xy[:, 0], xy[:, 1]
    dx, dy, e, _ = radial(w, h, p, tables, px, py)
    q = (p.ca_red, 0.0, p.ca_blue)[channel]
    sx, sy = source(px, py, dx, dy, e, q)
    return np.stack([sx, sy], axis=1).astype(F)


def _catmull_rom(t):
    t2 = t * t
    t3 = t2 * t
    return [((-t3 + F(2.0) * t2) - t) * F(0.5), ((F(3.0) * t3 - F(5.0) * t2) + F(2.0)) * F(0.5),
            ((F(-3.0) * t3 + F(4.0) * t2) + t) * F(0.5), (t3 - t2) * F(0.5)]


def _lerp(a, b, t):
    return a + t * (b - a)


def sample(plane, sx, sy, filt, anti_ring, border):
    """Steps 3 and 4 for one channel plane [H,W] at positions [H,W] -> (values [H,W], reads_nonfinite [H,W])."""
    h, w = plane.shape
    wf, hf = F(w), F(h)
    finite = np.isfinite(plane)
    val = np.where(finite, plane, F(0.0)).astype(F)
    with np.errstate(invalid="ignore"):
        inside = (sx >= 0) & (sx <= wf) & (sy >= 0) & (sy <= hf)
        cxs = np.where(sx > 0, np.where(sx < wf, sx, wf), F(0.0)).astype(F)
        cys = np.where(sy > 0, np.where(sy < hf, sy, hf), F(0.0)).astype(F)
    ux, uy = cxs - F(0.5), cys - F(0.5)
    flx, fly = np.floor(ux), np.floor(uy)
    ix, iy = flx.astype(np.int64), fly.astype(np.int64)
    fx, fy = ux - flx, uy - fly
    reads = np.zeros(plane.shape, bool)

    def tap(i, j):
        x = np.clip(ix + i, 0, w - 1)
        y = np.clip(iy + j, 0, h - 1)
        reads[...] |= ~finite[y, x]
        return val[y, x]
    with np.errstate(over="ignore", invalid="ignore"):
        if filt == BILINEAR:
            v00, v10, v01, v11 = tap(0, 0), tap(1, 0), tap(0, 1), tap(1, 1)
            v = _lerp(_lerp(v00, v10, fx), _lerp(v01, v11, fx), fy)
            centre = v00
        else:
            wx, wy = _catmull_rom(fx), _catmull_rom(fy)
            rows, inner = [], {}
            for j in range(4):
                t = [tap(i - 1, j - 1) for i in range(4)]
                rows.append((((wx[0] * t[0]) + (wx[1] * t[1])) + (wx[2] * t[2])) + (wx[3] * t[3]))
                if j in (1, 2):
                    inner[j] = (t[1], t[2])
            v = (((wy[0] * rows[0]) + (wy[1] * rows[1])) + (wy[2] * rows[2])) + (wy[3] * rows[3])
            centre = inner[1][0]
            if anti_ring:
                lo = hi = None
                for t in (inner[1][0], inner[1][1], inner[2][0], inner[2][1]):
                    lo = t if lo is None else np.where(t < lo, t, lo)
                    hi = t if hi is None else np.where(hi < t, t, hi)
                v = np.where(v < lo, lo, v)     # max(v, lo)
                v = np.where(hi < v, hi, v)     # min(., hi)
        v = np.where((fx == 0) & (fy == 0), centre, v).astype(F)
    if border == BLACK:
        v = np.where(inside, v, F(0.0)).astype(F)
        reads &= inside
    return v, reads


def lens(rad, p, tables, details=False):
    """ff_lens of rad [H,W,3] under the FfLensParams p with the tables (e, gain, r2_max) -> (rgb8, radiance[, details])."""
    rad = np.asarray(rad, F)
    h, w = rad.shape[:2]
    y, x = np.mgrid[0:h, 0:w]
    px, py = x.astype(F) + F(0.5), y.astype(F) + F(0.5)
    dx, dy, e, g = radial(w, h, p, tables, px, py)
    anti = bool(p.flags & ANTI_RING)
    out = np.zeros((h, w, 3), F)
    reads = np.zeros((h, w, 3), bool)
    pos = np.zeros((h, w, 3, 2), F)
    for c, q in enumerate((p.ca_red, 0.0, p.ca_blue)):
        sx, sy = source(px, py, dx, dy, e, q)
        v, r = sample(rad[..., c], sx, sy, p.filter, anti, p.border)
        with np.errstate(over="ignore", invalid="ignore"):
            out[..., c] = v * g
        reads[..., c] = r
        pos[..., c, 0], pos[..., c, 1] = sx, sy
    if details:
        return to_u8(out), out, dict(reads_nonfinite=reads, positions=pos, gain=g, e=e)
    return to_u8(out), out


# ---- the closed form, float64 -------------------------------------------------------------------------------------------------------

def model_f(k, s):
    t = s * s
    return s * (1.0 + k[0] * t + k[1] * t * t + k[2] * t * t * t)


def model_f_inverse(k, rho):
    """The s >= 0 with f(s) = rho on f's rising branch from 0, by bisection in float64 (rho: array)."""
    rho = np.asarray(rho, np.float64)
    lo = np.zeros_like(rho)
    hi = np.maximum(rho, 1.0e-30)
    for _ in range(80):  # grow until f(hi) >= rho (the cases' coefficients rise that far)
        short = model_f(k, hi) < rho
        if not short.any():
            break
        hi = np.where(short, hi * 1.25, hi)
    for _ in range(14):
        mid = 0.5 * (lo + hi)
        below = model_f(k, mid) < rho
        lo = np.where(below, mid, lo)
        hi = np.where(below, hi, mid)
    s = 0.5 * (lo + hi)
    for _ in range(5):  # Newton from 2^-14 of the bracket: quadratic, at float64's end after three steps
        t = s * s
        slope = 1.0 + 3.0 * k[0] * t + 5.0 * k[1] * t * t + 7.0 * k[2] * t * t * t
        s = np.clip(s - (model_f(k, s) - rho) / slope, lo, hi)
    exact = model_f(k, rho) == rho
    return np.where(exact, rho, s)


def model_source_radius(p, r):
    """The source radius (normalised, float64) of the output radius r under p: m(r / zoom)."""
    k = (float(p.k1), float(p.k2), float(p.k3))
    rho = np.asarray(r, np.float64) / float(p.zoom)
    return model_f(k, rho) if p.direction == UNDISTORT else model_f_inverse(k, rho)


def model_tables(p, r2_max):
    """e and gain at the FF_LENS_KNOTS + 1 knots in float64, as the header states them."""
    j = np.arange(KNOTS + 1, dtype=np.float64)
    r2 = r2_max * j / float(KNOTS)
    r = np.sqrt(r2)
    rho = r / float(p.zoom)
    src = model_source_radius(p, r)
    with np.errstate(invalid="ignore", divide="ignore"):
        e = src / r - 1.0
    e[0] = 1.0 / float(p.zoom) - 1.0
    lens_r = rho if p.direction == DISTORT else src
    fr = float(p.vignette_falloff) * lens_r
    c = 1.0 + fr * fr
    v = 1.0 / (c * c)
    gain = (1.0 - float(p.vignette)) + float(p.vignette) * v
    return e, (gain if p.direction == DISTORT else 1.0 / gain)


def model_map(w, h, p, xy, channel=1):
    """The source positions of the float64 positions xy [n,2] under the model itself (no table, no float32); channel: one of
    0, 1, 2, or a tuple of them for a tuple of results (the radial part is computed once)."""
    if isinstance(channel, tuple):
        green = model_map(w, h, p, xy, 1)
        c = np.array([float(F(0.5) * F(w) + F(p.center_x)), float(F(0.5) * F(h) + F(p.center_y))])
        # (1 + e)(1 + q) about c: the green position scaled
        return tuple(c + (green - c) * (1.0 + float((p.ca_red, 0.0, p.ca_blue)[ch])) for ch in channel)
    xy = np.asarray(xy, np.float64)
    cx = float(F(0.5) * F(w) + F(p.center_x))
    cy = float(F(0.5) * F(h) + F(p.center_y))
    d = np.sqrt(0.25 * (float(w) ** 2 + float(h) ** 2))
    dx, dy = xy[:, 0] - cx, xy[:, 1] - cy
    r = np.sqrt(dx * dx + dy * dy) / d
    src = model_source_radius(p, r)
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = np.where(r > 0, src / r, 1.0 / float(p.zoom))
    q = float((p.ca_red, 0.0, p.ca_blue)[channel])
    scale = ratio * (1.0 + q)
    return np.stack([cx + dx * scale, cy + dy * scale], axis=1)
