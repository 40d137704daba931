"""A numpy float32 restatement of ff_interpolate, written from the text in include/firefly/ff_api.h: test infrastructure only.

Every value is float32 and every expression is evaluated with the header's parentheses, so the kernels (ff_interpolate), the host
twin (ff_interpolate_host) and this file are held to one another bit for bit.  What the header prepares in double on the host - the
inverse of each camera's ray matrix by Gauss-Jordan elimination with partial pivoting, and pix_S - is done in Python floats here,
operation by operation.
"""
import ctypes as C
import math

import numpy as np

from gpupathtracer_amd import types as T

f32 = np.float32
BOTH, A_ONLY, B_ONLY, FILLED, FALLBACK = range(5)
HOLE = 3
IDENTITY = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0]], np.float32)


def ray_matrix32(camera):
    """ff_camera_ray_matrix(camera): 16 float32, column-major."""
    from gpupathtracer_amd import lib
    m = T.FfMat4()
    lib.load().ff_camera_ray_matrix(C.byref(camera), C.byref(m))
    return np.array(m.m[:], dtype=np.float32)


def invert4(m16):
    """The inverse of a column-major 4x4 matrix in double by Gauss-Jordan elimination with partial pivoting (the first largest
    pivot; the pivot row is divided first, then taken from every other row whose entry is not 0), rounded to float32."""
    a = [[float(m16[c * 4 + r]) for c in range(4)] + [1.0 if r == c else 0.0 for c in range(4)] for r in range(4)]
    for c in range(4):
        piv = c
        for r in range(c + 1, 4):
            if abs(a[r][c]) > abs(a[piv][c]):
                piv = r
        assert a[piv][c] != 0.0, "singular"
        a[c], a[piv] = a[piv], a[c]
        d = a[c][c]
        a[c] = [v / d for v in a[c]]
        for r in range(4):
            if r == c or a[r][c] == 0.0:
                continue
            f = a[r][c]
            a[r] = [v - f * p for v, p in zip(a[r], a[c])]
    return np.array([a[r][4 + c] for c in range(4) for r in range(4)], dtype=np.float64).astype(np.float32)


def pixel_size(camera):
    """pix_S: 2 tan(m_fov / 2) / m_screenHeight in double, rounded."""
    return f32(2.0 * math.tan(float(camera.m_fov) * (3.14159265358979323846 / 180.0) * 0.5) / float(camera.m_screenHeight))


def _project(P, X, sw, sh):
    x, y, z = X[..., 0], X[..., 1], X[..., 2]
    qx = (P[0] * x + P[4] * y) + (P[8] * z + P[12])
    qy = (P[1] * x + P[5] * y) + (P[9] * z + P[13])
    qw = (P[3] * x + P[7] * y) + (P[11] * z + P[15])
    ok = qw > 0
    sq = np.where(ok, qw, f32(1))
    return ok, (qx / sq + f32(1)) * f32(0.5) * sw, (f32(1) - qy / sq) * f32(0.5) * sh


class _Mean:
    """ff_upscale's "mean" over taps named one after the other, per pixel."""

    def __init__(self, shape):
        self.n = np.zeros(shape, np.int32)
        self.w = np.zeros(shape, np.float32)
        self.c0 = np.zeros(shape + (3,), np.float32)
        self.s = np.zeros(shape + (3,), np.float32)

    def add(self, counts, w, c):
        first, later = counts & (self.n == 0), counts & (self.n > 0)
        self.c0 = np.where(first[..., None], c, self.c0)
        self.s = np.where(later[..., None], self.s + w[..., None] * (c - self.c0), self.s)
        self.w = np.where(counts, self.w + w, self.w)
        self.n = self.n + counts

    def get(self):
        safe = np.where(self.n > 1, self.w, f32(1))
        return np.where((self.n == 1)[..., None], self.c0, self.c0 + self.s / safe[..., None])


def _blend(t, a, b):
    if t == 0:
        return a.copy()
    mixed = b if t == 1 else (f32(1) - t) * a + t * b
    return np.where(a == b, a, mixed)


def _fetch(S, cam_mid, cam, W, H, t, tol, x_p, g, k, rad, pos, ids, maps):
    """Steps 1 and 2 for one source: (valid [H,W], c [H,W,3])."""
    ys, xs = np.mgrid[0:H, 0:W]
    xf, yf = xs.astype(np.float32), ys.astype(np.float32)
    hit = g >= 0
    ok = np.ones((H, W), bool)
    identity = np.ones((H, W), bool)
    xh = x_p.copy()
    if maps is not None:
        n = maps.shape[0]
        ok &= ~hit | (g < n)
        for gi in range(n):
            a = maps[gi, S]
            if a.tobytes() == IDENTITY.tobytes():
                continue
            on = hit & (g == gi)
            identity &= ~on
            px, py, pz = x_p[..., 0], x_p[..., 1], x_p[..., 2]
            moved = np.stack([(a[r, 0] * px + a[r, 1] * py) + (a[r, 2] * pz + a[r, 3]) for r in range(3)], -1)
            xh = np.where(on[..., None], moved, xh)
    M = ray_matrix32(cam_mid)
    inv_mid, inv_s = invert4(M), invert4(ray_matrix32(cam))
    sw, sh, far = f32(cam_mid.m_screenWidth), f32(cam_mid.m_screenHeight), f32(cam_mid.m_farClip)
    rest = (bytes(cam) == bytes(cam_mid)) & identity
    ok_b, bx, by = _project(inv_mid, x_p, sw, sh)
    bx, by, ok_b = np.where(hit, bx, xf), np.where(hit, by, yf), ok_b | ~hit
    Px, Py = (xf / sw) * f32(2) - f32(1), f32(1) - (yf / sh) * f32(2)
    v0, v1, v2 = Px * far, Py * far, f32(1) * far
    far_point = np.stack([(M[r] * v0 + M[4 + r] * v1) + (M[8 + r] * v2 + M[12 + r] * v2) for r in range(3)], -1)
    X = np.where(hit[..., None], xh, far_point)
    ok_s, fx, fy = _project(inv_s, X, f32(cam.m_screenWidth), f32(cam.m_screenHeight))
    hx, hy = xf + (fx - bx), yf + (fy - by)
    inside = (hx >= 0) & (hy >= 0) & (hx <= f32(W - 1)) & (hy <= f32(H - 1))
    ok &= rest | (ok_b & ok_s & inside)
    hx, hy = np.where(rest, xf, np.where(ok, hx, f32(0))), np.where(rest, yf, np.where(ok, hy, f32(0)))
    # 2 taps
    flx, fly = np.floor(hx), np.floor(hy)
    i0, j0 = flx.astype(np.int64), fly.astype(np.int64)
    tx, ty = hx - flx, hy - fly
    bu, bv = (f32(1) - tx, tx), (f32(1) - ty, ty)
    e = xh - np.array([cam.m_position.x, cam.m_position.y, cam.m_position.z], np.float32)
    D2 = (e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2]
    pix = pixel_size(cam)
    limit = (tol * tol) * (D2 * (pix * pix))
    mean = _Mean((H, W))
    for dj in range(2):
        jy = np.clip(j0 + dj, 0, H - 1)
        for di in range(2):
            ix = np.clip(i0 + di, 0, W - 1)
            b = bu[di] * bv[dj]
            c = rad[jy, ix]
            d = pos[jy, ix] - xh
            d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
            counts = ok & (b > 0) & (ids[jy, ix, 0] == g) & (ids[jy, ix, 2] == k) & np.isfinite(c).all(-1) & (~hit | (d2 <= limit))
            mean.add(counts, b, c)
    return mean.n > 0, mean.get()


def interpolate_ref(mid, a, b, t=0.5, surface_tolerance=4.0, fill_radius=4, geom_maps=None):
    """mid = (camera, position, ids), a and b = (camera, radiance, position, ids); geom_maps [n,2,3,4] float32 or None
    -> (radiance [H,W,3] float32, rgb8 [H,W,3] uint8, counts [5], state [H,W])."""
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        return _interpolate_ref(mid, a, b, f32(t), f32(surface_tolerance), int(fill_radius), geom_maps)


def _interpolate_ref(mid, a, b, t, tol, r, geom_maps):
    cam_mid = mid[0]
    x_p, ids_p = np.asarray(mid[1], np.float32), np.asarray(mid[2], np.int32)
    H, W = ids_p.shape[:2]
    g, k = ids_p[..., 0], ids_p[..., 2]
    maps = None if geom_maps is None else np.asarray(geom_maps, np.float32)
    got = []
    for S, src in enumerate((a, b)):
        got.append(_fetch(S, cam_mid, src[0], W, H, t, tol, x_p, g, k, np.asarray(src[1], np.float32), np.asarray(src[2], np.float32),
                          np.asarray(src[3], np.int32), maps))
    (va, ca), (vb, cb) = got
    # 3 combine
    o = np.where((va & vb)[..., None], _blend(t, ca, cb), np.where(va[..., None], ca, cb))
    state = np.where(va & vb, BOTH, np.where(va, A_ONLY, np.where(vb, B_ONLY, HOLE)))
    hole = state == HOLE
    o = np.where(hole[..., None], f32(0), o)
    # 4 fill
    mean = _Mean((H, W))
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            if dx == 0 and dy == 0:
                continue
            ys, xs = np.mgrid[0:H, 0:W]
            qy, qx = ys + dy, xs + dx
            inside = (qx >= 0) & (qy >= 0) & (qx < W) & (qy < H)
            qy, qx = np.clip(qy, 0, H - 1), np.clip(qx, 0, W - 1)
            donor = hole & inside & ~hole[qy, qx] & (g[qy, qx] == g) & (k[qy, qx] == k)
            w = np.full((H, W), f32(1) / f32(dx * dx + dy * dy), np.float32)
            mean.add(donor, w, o[qy, qx])
    filled = hole & (mean.n > 0)
    fallback = hole & ~filled
    out = np.where(filled[..., None], mean.get(), o)
    out = np.where(fallback[..., None], _blend(t, np.asarray(a[1], np.float32), np.asarray(b[1], np.float32)), out).astype(np.float32)
    state = np.where(filled, FILLED, np.where(fallback, FALLBACK, state))
    counts = np.array([(state == s).sum() for s in range(5)], np.uint32)
    return out, rgb8_of(out), counts, state


def rgb8_of(radiance):
    """The project's 8-bit rule: trunc(clamp(v * 255)) in float32, NaN -> 0."""
    with np.errstate(invalid="ignore", over="ignore"):
        s = np.asarray(radiance, dtype=np.float32) * f32(255.0)
        return np.where(s > 0, np.minimum(s, f32(255.0)), f32(0)).astype(np.uint8)


def same_bits(x, y):
    """Two float32 arrays agree bit for bit (NaN payloads aside: a NaN matches a NaN)."""
    x, y = np.asarray(x, np.float32), np.asarray(y, np.float32)
    return x.shape == y.shape and bool(((x.view(np.uint32) == y.view(np.uint32)) | (np.isnan(x) & np.isnan(y))).all())
