"""A numpy float32 restatement of ff_despeckle as include/firefly/ff_api.h defines it: the measure per pixel, the rank-th largest
luminance among the neighbours on the same geometry by a sort per pixel over the padded window, the clamp, the bytes and the count.
Every float32 operation is its own numpy operation (no fused multiply-add), in the header's order."""
import numpy as np

F = np.float32
EMITTER = 0          # FF_BXDF_EMITTER
DEMODULATE = 1       # FF_DESPECKLE_DEMODULATE_ALBEDO
STEPS = 64           # how often step 3 lowers s before it sets it to 0


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


def luminance(rad, albedo, flags=DEMODULATE):
    """Step 1's l of [..., 3] radiance."""
    rad = np.asarray(rad, F)
    c = rad.copy()
    with np.errstate(all="ignore"):
        if flags & DEMODULATE:
            albedo = np.asarray(albedo, F)
            pos = albedo > 0
            c[pos] = rad[pos] / albedo[pos]
        return ((F(0.2126) * c[..., 0] + F(0.7152) * c[..., 1]) + F(0.0722) * c[..., 2]).astype(F)


def measure(rad, albedo, ids, flags=DEMODULATE):
    """Step 1: (l [H,W] float32, g [H,W] int32 with -1 where the pixel does not count)."""
    rad = np.asarray(rad, F)
    ids = np.asarray(ids, np.int32)
    ok = (ids[..., 0] >= 0) & (ids[..., 2] != EMITTER) & np.isfinite(rad).all(axis=-1)
    if flags & DEMODULATE:
        ok &= ~np.isnan(np.asarray(albedo, F)).any(axis=-1)
    l = luminance(rad, albedo, flags)
    ok &= np.isfinite(l)
    return l, np.where(ok, ids[..., 0], -1).astype(np.int32)


def yardstick(l, g, radius, rank):
    """Step 2: (n [H,W] the number of neighbours, m [H,W] the rank-th largest of their l; -inf where there are fewer)."""
    h, w = l.shape
    r = radius
    lp = np.full((h + 2 * r, w + 2 * r), -np.inf, F)
    gp = np.full((h + 2 * r, w + 2 * r), -1, np.int32)
    lp[r:r + h, r:r + w] = l
    gp[r:r + h, r:r + w] = g
    vals, n = [], np.zeros((h, w), np.int32)
    for dy in range(2 * r + 1):
        for dx in range(2 * r + 1):
            if dx == r and dy == r:
                continue
            same = (gp[dy:dy + h, dx:dx + w] == g) & (g >= 0)
            n += same
            vals.append(np.where(same, lp[dy:dy + h, dx:dx + w], F(-np.inf)))
    ordered = np.sort(np.stack(vals), axis=0)  # ascending
    return n, ordered[len(vals) - rank]


def despeckle(rad, albedo, ids, radius=1, rank=2, min_neighbours=3, threshold=2.0, floor=0.0, flags=DEMODULATE, details=False):
    """-> (rgb8 [H,W,3] uint8, out [H,W,3] float32, clamped); with details also a dict of l, g, n, m, limit and the clamped mask."""
    rad = np.asarray(rad, F)
    l, g = measure(rad, albedo, ids, flags)
    n, m = yardstick(l, g, radius, rank)
    with np.errstate(all="ignore"):
        limit = F(threshold) * m
        limit = np.where(limit > F(floor), limit, F(floor)).astype(F)
        hit = (g >= 0) & (n >= min_neighbours) & (l > 0) & (l > limit)
        # the clamped pixels alone from here: s, the products, and s lowered a float32 at a time while the output measures above
        rad_x, limit_x = rad[hit], limit[hit]
        alb_x = np.asarray(albedo, F)[hit] if flags & DEMODULATE else None
        s = (limit_x / l[hit]).astype(F)
        steps = np.zeros(s.shape, np.int32)
        while True:
            out_x = (rad_x * s[:, None]).astype(F)
            over = (luminance(out_x, alb_x, flags) > limit_x) & (s > 0)
            if not over.any():
                break
            lower = (s.view(np.uint32) - np.uint32(1)).view(F)
            s = np.where(over, np.where(steps < STEPS, lower, F(0.0)), s).astype(F)
            steps += over
        out = rad.copy()
        out[hit] = out_x
    result = (to_u8(out), out, int(hit.sum()))
    if details:
        lowered = np.zeros(l.shape, np.int32)
        lowered[hit] = steps
        return result + (dict(l=l, g=g, n=n, m=m, limit=limit, hit=hit, lowered=lowered),)
    return result
