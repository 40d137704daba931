"""ff_depth_of_field in numpy float32, written from the operator in include/firefly/ff_api.h (steps 1-5), not from the C++: every
expression is evaluated in float32 as the header parenthesises it; numpy never fuses a multiply with an add, and its float32 sqrt
and division are correctly rounded, so the library has to agree bit for bit.  coc_scale comes in as a number: no tangent here."""
import numpy as np

F = np.float32
FLT_MAX = np.finfo(np.float32).max


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def clamp01(v):
    return np.where(v < F(0), F(0), np.where(v > F(1), F(1), v)).astype(np.float32)


def finite3(c):
    return np.isfinite(c).all(axis=-1)


def pack(position, depth, origin, forward, focus_distance, coc_scale, k):
    """Step 1 -> (l [H,W], zk [H,W])."""
    with np.errstate(all="ignore"):
        p = np.asarray(position, np.float32)
        o = np.asarray(origin, np.float32)
        f = np.asarray(forward, np.float32)
        e = (p - o).astype(np.float32)
        z = ((e[..., 0] * f[0] + e[..., 1] * f[1]) + e[..., 2] * f[2]).astype(np.float32)
        depth = np.asarray(depth, np.float32)
        hit = np.isfinite(depth) & (depth > F(0)) & np.isfinite(z) & (z > F(1e-6))
        iz = np.where(hit, F(1) / np.where(hit, z, F(1)), F(0)).astype(np.float32)
        fi = F(1) / F(focus_distance)
        l = (F(coc_scale) * np.abs(fi - iz)).astype(np.float32)
        l = np.where(l > F(k), F(k), l).astype(np.float32)
        zk = np.where(hit, z, FLT_MAX).astype(np.float32)
    return l, zk


def tile_max(l, k):
    """Step 2 -> T [tiles_y, tiles_x]."""
    h, w = l.shape
    ty, tx = (h + k - 1) // k, (w + k - 1) // k
    T = np.zeros((ty, tx), np.float32)
    for j in range(ty):
        for i in range(tx):
            T[j, i] = l[j * k:min((j + 1) * k, h), i * k:min((i + 1) * k, w)].max()
    return T


def neighbour_max(T):
    """Step 3 -> N, the shape of T."""
    ty, tx = T.shape
    N = np.zeros_like(T)
    for j in range(ty):
        for i in range(tx):
            N[j, i] = T[max(j - 1, 0):min(j + 2, ty), max(i - 1, 0):min(i + 2, tx)].max()
    return N


def jitters(h, w):
    x = np.arange(w, dtype=np.uint32)[None, :]
    y = np.arange(h, dtype=np.uint32)[:, None]
    with np.errstate(over="ignore"):
        hh = (x * np.uint32(0x9E3779B1)) ^ (y * np.uint32(0x85EBCA77))
        hh = hh ^ (hh >> np.uint32(15))
        hh = hh * np.uint32(0x2C1B3C6D)
        hh = hh ^ (hh >> np.uint32(12))
        h2 = hh * np.uint32(0x9E3779B1)
    u = lambda v: ((v >> np.uint32(8)).astype(np.float32) * F(2.0 ** -24) - F(0.5)).astype(np.float32)  # noqa: E731
    return u(hh), u(h2)


def cover(d, l):
    return clamp01((l - d) + F(0.5))


def intensity(l):
    q = np.where(l > F(0.5), l, F(0.5)).astype(np.float32)
    return (F(1) / (q * q)).astype(np.float32)


def to_u8(v):
    s = np.asarray(v, np.float32) * F(255)
    with np.errstate(invalid="ignore"):
        t = np.where(s >= F(255), F(255), np.where(s > F(0), s, F(0)))  # (NaN: neither comparison holds -> 0)
    return np.trunc(t).astype(np.uint8)


def depth_of_field(radiance, position, depth, origin, forward, focus_distance=1.0, coc_scale=0.0, max_radius=16, grid=4, depth_extent=0.1,
                   exclude=None):
    """Steps 1-5 -> (rgb8 [H,W,3] uint8, out [H,W,3] float32).  exclude: an [H,W] mask of pixels that never count as taps (for the
    non-finite test's comparison image)."""
    c = np.ascontiguousarray(radiance, np.float32)
    h, w = c.shape[:2]
    k, g = int(max_radius), int(grid)
    l, z = pack(position, depth, origin, forward, focus_distance, coc_scale, k)
    N = neighbour_max(tile_max(l, k))
    ys, xs = np.mgrid[0:h, 0:w]
    n = N[ys // k, xs // k]
    usable = finite3(c)
    if exclude is not None:
        usable = usable & ~exclude
    active = (~(n <= F(0.5))) & finite3(c)
    jx, jy = jitters(h, w)
    asum = np.zeros((h, w), np.float32)
    s = np.zeros((h, w, 3), np.float32)
    with np.errstate(all="ignore"):
        for b in range(-g, g + 1):
            dy = np.floor(n * ((F(b) + jy) / F(g)) + F(0.5)).astype(np.int64)
            for a in range(-g, g + 1):
                if a * a + b * b > g * g:
                    continue
                dx = np.floor(n * ((F(a) + jx) / F(g)) + F(0.5)).astype(np.int64)
                qx, qy = xs + dx, ys + dy
                ok = active & ~((dx == 0) & (dy == 0)) & (qx >= 0) & (qy >= 0) & (qx < w) & (qy < h)
                qx, qy = np.clip(qx, 0, w - 1), np.clip(qy, 0, h - 1)
                ok = ok & usable[qy, qx]
                cY, lY, zY = c[qy, qx], l[qy, qx], z[qy, qx]
                d = np.sqrt((dx * dx + dy * dy).astype(np.float32))
                f = clamp01(F(1) - (zY - z) / F(depth_extent))
                m = np.where(lY < l, lY, l).astype(np.float32)
                wgt = ((f * cover(d, lY) + (F(1) - f) * cover(d, m)) * intensity(lY)).astype(np.float32)
                s = np.where(ok[..., None], s + wgt[..., None] * (cY - c), s).astype(np.float32)
                asum = np.where(ok, asum + wgt, asum).astype(np.float32)
        w0 = intensity(l)
        blurred = np.where(s != F(0), c + s / (w0 + asum)[..., None], c).astype(np.float32)  # (a sum of 0 keeps the centre's bits)
    out = np.where(active[..., None], blurred, c).astype(np.float32)
    return to_u8(out), out
