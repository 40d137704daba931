"""ff_motion_blur in numpy float32, written from the operator in include/firefly/ff_api.h (steps 1-5), not from the C++: every
expression is evaluated in float32 as the header parenthesises it; numpy never fuses a multiply with an add, and its float32 sqrt
and division are correctly rounded, so the library has to agree bit for bit."""
import numpy as np

F = np.float32
FLT_MAX = np.finfo(np.float32).max


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def clamp01(v):
    return np.where(v < F(0), F(0), np.where(v > F(1), F(1), v)).astype(np.float32)


def finite3(c):
    return np.isfinite(c).all(axis=-1)


def pack(motion, depth, shutter, k):
    """Step 1 -> (v [H,W,2], l [H,W], z [H,W])."""
    with np.errstate(all="ignore"):
        hs = F(0.5) * F(shutter)
        v = np.asarray(motion, np.float32) * hs
        bad = ~np.isfinite(v).all(axis=-1)
        v = np.where(bad[..., None], F(0), v).astype(np.float32)
        l = np.sqrt(v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1])
        big = l > F(k)
        s = F(k) / np.where(big, l, F(1))
        v = np.where(big[..., None], v * s[..., None], v).astype(np.float32)
        l = np.where(big, np.sqrt(v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]), l).astype(np.float32)
        depth = np.asarray(depth, np.float32)
        z = np.where(np.isfinite(depth) & (depth > F(0)), depth, FLT_MAX).astype(np.float32)
    return v, l, z


def _first_largest(q):
    """Index of the first largest value of a 1-D float32 array of values >= 0 (np.argmax returns the first)."""
    return int(np.argmax(q))


def tile_max(v, l, k):
    """Step 2 -> T [tiles_y, tiles_x, 3] = {v.x, v.y, l}."""
    h, w = l.shape
    ty, tx = (h + k - 1) // k, (w + k - 1) // k
    q = v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]
    T = np.zeros((ty, tx, 3), np.float32)
    for j in range(ty):
        for i in range(tx):
            ys, xs = slice(j * k, min((j + 1) * k, h)), slice(i * k, min((i + 1) * k, w))
            n = _first_largest(q[ys, xs].reshape(-1))  # (row-major within the tile)
            T[j, i, :2] = v[ys, xs].reshape(-1, 2)[n]
            T[j, i, 2] = l[ys, xs].reshape(-1)[n]
    return T


def neighbour_max(T):
    """Step 3 -> N, the shape of T."""
    ty, tx = T.shape[:2]
    q = T[..., 0] * T[..., 0] + T[..., 1] * T[..., 1]
    N = np.zeros_like(T)
    for j in range(ty):
        for i in range(tx):
            ys, xs = slice(max(j - 1, 0), min(j + 2, ty)), slice(max(i - 1, 0), min(i + 2, tx))
            n = _first_largest(q[ys, xs].reshape(-1))  # (row-major over the tiles that exist)
            N[j, i] = T[ys, xs].reshape(-1, 3)[n]
    return N


def jitter(h, w):
    x = np.arange(w, dtype=np.uint32)[None, :]
    y = np.arange(h, dtype=np.uint32)[:, None]
    with np.errstate(over="ignore"):
        hh = (x * np.uint32(0x9E3779B1)) ^ (y * np.uint32(0x85EBCA77))
        hh = hh ^ (hh >> np.uint32(15))
        hh = hh * np.uint32(0x2C1B3C6D)
        hh = hh ^ (hh >> np.uint32(12))
    return ((hh >> np.uint32(8)).astype(np.float32) * F(2.0 ** -24) - F(0.5)).astype(np.float32)


def soft(a, b, extent):
    return clamp01(F(1) - (a - b) / F(extent))


def cone(d, l):
    pos = l > F(0)
    return np.where(pos, clamp01(F(1) - d / np.where(pos, l, F(1))), F(0)).astype(np.float32)


def cylinder(d, l):
    pos = l > F(0)
    ls = np.where(pos, l, F(1)).astype(np.float32)
    lo, hi = F(0.95) * ls, F(1.05) * ls
    u = clamp01((d - lo) / (hi - lo))
    return np.where(pos, F(1) - ((u * u) * (F(3) - (F(2) * u))), F(0)).astype(np.float32)


def to_u8(v):
    s = np.asarray(v, np.float32) * F(255)
    with np.errstate(invalid="ignore"):
        t = np.where(s >= F(255), F(255), np.where(s > F(0), s, F(0)))  # (NaN: neither comparison holds -> 0)
    return np.trunc(t).astype(np.uint8)


def motion_blur(radiance, motion, depth, shutter=0.5, max_radius=16, samples=15, depth_extent=0.1, exclude=None):
    """Steps 1-5 -> (rgb8 [H,W,3] uint8, out [H,W,3] float32).  exclude: an [H,W] mask of pixels that never count as taps (for the
    non-finite test's comparison image)."""
    c = np.ascontiguousarray(radiance, np.float32)
    h, w = c.shape[:2]
    k, S = int(max_radius), int(samples)
    v, l, z = pack(motion, depth, shutter, k)
    N = neighbour_max(tile_max(v, l, k))
    ys, xs = np.mgrid[0:h, 0:w]
    n = N[ys // k, xs // k]                    # per pixel: {vn.x, vn.y, ln}
    usable = finite3(c)
    if exclude is not None:
        usable = usable & ~exclude
    active = (~(n[..., 2] <= F(0.5))) & finite3(c)
    j = jitter(h, w)
    asum = np.zeros((h, w), np.float32)
    s = np.zeros((h, w, 3), np.float32)
    with np.errstate(all="ignore"):
        for i in range(S):
            t = ((((F(i) + j) + F(1)) / F(S + 1)) * F(2) - F(1)).astype(np.float32)
            dx = np.floor(n[..., 0] * t + F(0.5)).astype(np.int64)
            dy = np.floor(n[..., 1] * t + F(0.5)).astype(np.int64)
            qx, qy = xs + dx, ys + dy
            ok = active & ~((dx == 0) & (dy == 0)) & (qx >= 0) & (qy >= 0) & (qx < w) & (qy < h)
            qx, qy = np.clip(qx, 0, w - 1), np.clip(qy, 0, h - 1)
            ok = ok & usable[qy, qx]
            cY, lY, zY = c[qy, qx], l[qy, qx], z[qy, qx]
            d = np.sqrt((dx * dx + dy * dy).astype(np.float32))
            f, b = soft(zY, z, depth_extent), soft(z, zY, depth_extent)
            a = ((f * cone(d, lY) + b * cone(d, l)) + (cylinder(d, lY) * cylinder(d, l)) * F(2)).astype(np.float32)
            s = np.where(ok[..., None], s + a[..., None] * (cY - c), s).astype(np.float32)
            asum = np.where(ok, asum + a, asum).astype(np.float32)
        w0 = F(1) / np.maximum(l, F(0.5))
        blurred = np.where(s != F(0), c + s / (w0 + asum)[..., None], c).astype(np.float32)  # (a sum of 0 keeps the centre's bits)
    out = np.where(active[..., None], blurred, c).astype(np.float32)
    return to_u8(out), out
