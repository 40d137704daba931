"""A numpy float32 restatement of ff_sharpen as include/firefly/ff_api.h defines it: the compression per pixel, the four cross taps
with the image edge giving the pixel itself, the limited lobe, the noise term, the application and the bytes.  Every float32
operation is its own numpy operation (no fused multiply-add), in the header's order; min and max are np.where as the header
defines them."""
import numpy as np

F = np.float32
NOISE_AWARE = 1          # FF_SHARPEN_NOISE_AWARE
LIMIT = F(0.1875)
CAP = F(0.99999988)      # 1 - 2^-23
MAXC = F(8388608.0)      # 2^23
assert CAP == F(1.0) - F(2.0 ** -23) and MAXC == F(2.0 ** 23)


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


def fmin(a, b):
    """min(a, b) = b < a ? b : a"""
    return np.where(b < a, b, a).astype(F)


def fmax(a, b):
    """max(a, b) = a < b ? b : a"""
    return np.where(a < b, b, a).astype(F)


def compress(rad):
    """Step 1: (t [H,W,3], L [H,W], usable [H,W]); t and L are 0 where the pixel is not usable."""
    rad = np.asarray(rad, F)
    with np.errstate(all="ignore"):
        m = fmax(fmax(rad[..., 0], rad[..., 1]), rad[..., 2])
        usable = np.isfinite(rad).all(axis=-1) & (rad >= 0).all(axis=-1) & (m <= MAXC)
        d = (F(1.0) + m).astype(F)
        t = ((rad / d[..., None]).astype(F) + F(0.0)).astype(F)
        t[~usable] = 0
        L = ((F(0.2126) * t[..., 0] + F(0.7152) * t[..., 1]).astype(F) + F(0.0722) * t[..., 2]).astype(F)
    return t, L, usable


def taps(plane):
    """Step 2: the planes of B, D, F, H for a [H,W,...] plane; a tap outside the image is E itself."""
    b, d, f, h = plane.copy(), plane.copy(), plane.copy(), plane.copy()
    b[1:] = plane[:-1]
    d[:, 1:] = plane[:, :-1]
    f[:, :-1] = plane[:, 1:]
    h[:-1] = plane[1:]
    return b, d, f, h


def sharpen(rad, strength=0.5, flags=NOISE_AWARE, details=False):
    """-> (rgb8 [H,W,3] uint8, out [H,W,3] float32); with details also a dict of the masks and intermediates."""
    rad = np.ascontiguousarray(rad, F)
    strength = F(strength)
    t, L, usable = compress(rad)
    tb, td, tf, th = taps(t)
    ub, ud, uf, uh = taps(usable)
    Lb, Ld, Lf, Lh = taps(L)
    all_usable = usable & ub & ud & uf & uh
    same = ((tb == t) & (td == t) & (tf == t) & (th == t)).all(axis=-1)
    with np.errstate(all="ignore"):
        # step 3
        mn = fmin(fmin(tb, td), fmin(tf, th))
        mx = fmax(fmax(tb, td), fmax(tf, th))
        first = (-(mn / (F(4.0) * mx).astype(F)).astype(F)).astype(F)
        second = ((F(1.0) - mx).astype(F) / ((F(4.0) * mn).astype(F) - F(4.0)).astype(F)).astype(F)
        lobe_k = np.where(mx == 0, -LIMIT, fmax(first, second)).astype(F)
        widest = fmax(fmax(lobe_k[..., 0], lobe_k[..., 1]), lobe_k[..., 2])
        inner = fmin(widest, np.zeros_like(widest))
        limited = fmax(np.full_like(widest, -LIMIT), inner)
        lobe = (limited * strength).astype(F)
        # step 4
        rng = np.zeros_like(L)
        if flags & NOISE_AWARE:
            n = ((F(0.25) * (((Lb + Ld).astype(F) + Lf).astype(F) + Lh).astype(F)).astype(F) - L).astype(F)
            hi = fmax(fmax(fmax(fmax(L, Lb), Ld), Lf), Lh)
            lo = fmin(fmin(fmin(fmin(L, Lb), Ld), Lf), Lh)
            rng = (hi - lo).astype(F)
            a = fmin((np.abs(n) / rng).astype(F), np.ones_like(rng))
            scaled = (lobe * (F(1.0) - (F(0.5) * a).astype(F)).astype(F)).astype(F)
            lobe = np.where(rng > 0, scaled, lobe).astype(F)
        # step 5
        den = ((F(4.0) * lobe).astype(F) + F(1.0)).astype(F)
        total = (((tb + td).astype(F) + tf).astype(F) + th).astype(F)
        raw = (((lobe[..., None] * total).astype(F) + t).astype(F) / den[..., None]).astype(F)
        o = fmin(fmax(raw, np.zeros_like(raw)), np.full_like(raw, CAP))
        M = fmax(fmax(o[..., 0], o[..., 1]), o[..., 2])
        back = (o / (F(1.0) - M).astype(F)[..., None]).astype(F)
    active = all_usable & ~same & (lobe != 0)
    out = rad.copy()
    out[active] = back[active]
    result = (to_u8(out), out)
    if details:
        judged = all_usable & ~same
        return result + (dict(t=t, L=L, usable=usable, all_usable=all_usable, same=same, judged=judged, active=active, lobe=lobe, mx=mx, mn=mn, raw=raw, o=o,
                              range=rng),)
    return result
