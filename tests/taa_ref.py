"""CPU reference of the temporal anti-aliasing resolve (ff_taa): test infrastructure only.

TaaRef.step is one call of include/firefly/ff_api.h's ff_taa in float64 numpy, written from the formulas there: the motion through
the G-buffer, the previous camera and the geometries' rigid motion, the validity of the history, its Catmull-Rom (or bilinear)
resampling, the YCoCg neighbourhood clamp and the blend.  It keeps the history between calls as the state does.  Besides the
output it reports, per pixel, whether a validity bound or the nearest-tap decision floor(h + 0.5) was within 1e-5 (relative) of its threshold: such
pixels may legitimately decide the other way in float32.  `tainted` adds every pixel whose history reads one of them with a
nonzero weight, across calls.

Non-finite input follows ff_api.h: the clamp box is taken over the finite samples of the 3x3 neighbourhood, and a resampled
history that is not finite (a zero weight times a stored NaN included) is not valid.
"""
import numpy as np

from gpupathtracer_amd import types as T
from temporal_ref import ray_matrix

NEAR = 1e-5
MAX_LENGTH = 4096.0
# RGB -> YCoCg and back (rows act on column vectors)
YCOCG = np.array([[0.25, 0.5, 0.25], [0.5, 0.0, -0.5], [-0.25, 0.5, -0.25]])
RGB = np.array([[1.0, 1.0, -1.0], [1.0, 0.0, 1.0], [1.0, -1.0, -1.0]])


def catmull_rom(t):
    """The four weights of taps floor(h) - 1 .. floor(h) + 2 for fraction t (array), stacked on a new last axis."""
    t = np.asarray(t, dtype=np.float64)
    t2, t3 = t * t, t * t * t
    return np.stack([(-t3 + 2 * t2 - t) / 2, (3 * t3 - 5 * t2 + 2) / 2, (-3 * t3 + 4 * t2 + t) / 2, (t3 - t2) / 2], -1)


def _params(p):
    if isinstance(p, dict):
        return dict(p)
    return {f: getattr(p, f) for f, _ in T.FfTaaParams._fields_}


def _near(v, at):
    return np.abs(v - at) <= NEAR * np.maximum(1.0, np.abs(at))


def neighbourhood_box(c, gamma):
    """(lo, hi) per pixel and YCoCg channel: the 3x3 clamp box of ff_taa over the image c [H,W,3] (borders clamped), over the
    samples whose r, g, b are all finite."""
    H, W = c.shape[:2]
    pad = np.pad(c, ((1, 1), (1, 1), (0, 0)), mode="edge")
    rgb = np.stack([pad[dy:dy + H, dx:dx + W] for dy in range(3) for dx in range(3)])
    fin = np.isfinite(rgb).all(-1, keepdims=True)
    taps = np.where(fin, rgb, 0.0) @ YCOCG.T
    n = fin.sum(0)
    mu = taps.sum(0) / n
    sigma = np.sqrt(np.fmax(0.0, (taps * taps).sum(0) / n - mu * mu))
    lo, hi = np.where(fin, taps, np.inf).min(0), np.where(fin, taps, -np.inf).max(0)
    return np.fmax(lo, mu - gamma * sigma), np.fmin(hi, mu + gamma * sigma)


class TaaRef:
    """ff_taa with a history of its own; step() is one call."""

    def __init__(self):
        self.reset()

    def reset(self):
        self.prev = None

    def step(self, radiance, gbuffer, camera, models, p, replaced=()):
        """radiance [H,W,3]; gbuffer: ff_gbuffer's dict (position, ids) for `camera` and the frame's jitter; models:
        temporal_ref.scene_models() of the scene as it is now; p: an FfTaaParams or a dict of its fields; replaced: geometries
        whose mesh ff_update_mesh replaced since the last call.  Returns a dict: out [H,W,3] float64, motion [H,W,2],
        length [H,W], valid [H,W] bool, near [H,W] bool, tainted [H,W] bool."""
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            return self._step(radiance, gbuffer, camera, models, p, replaced)

    def _step(self, radiance, gbuffer, camera, models, p, replaced):
        p = _params(p)
        c = np.asarray(radiance, dtype=np.float32).astype(np.float64)
        H, W = c.shape[:2]
        geom = np.asarray(gbuffer["ids"])[..., 0]
        hit = geom >= 0
        x = np.asarray(gbuffer["position"], dtype=np.float32).astype(np.float64)
        ys, xs = np.mgrid[0:H, 0:W].astype(np.float64)
        M = ray_matrix(camera)
        sw, sh = np.float64(np.float32(camera.m_screenWidth)), np.float64(np.float32(camera.m_screenHeight))
        motion = np.zeros((H, W, 2))
        valid = np.zeros((H, W), bool)
        near = np.zeros((H, W), bool)
        taint = np.zeros((H, W), bool)
        cam_bytes = bytes(camera)
        prev = self.prev
        out, length = c.copy(), np.ones((H, W))
        if prev is not None and prev["shape"] == (H, W):
            moved = np.zeros((H, W), bool)
            rep = np.zeros((H, W), bool)
            known = ~hit | (geom < len(models))
            xh = x.copy()
            for k, (mod, inv) in enumerate(models):
                on = hit & (geom == k)
                if k in replaced:
                    rep |= on
                pm = prev["models"][k][0] if k < len(prev["models"]) else None
                if pm is None or np.array_equal(pm[:3], mod[:3]):
                    continue
                A = pm @ inv
                moved |= on
                xh[on] = x[on] @ A[:3, :3].T + A[:3, 3]
            # the base: P(M_cur, x_p) for a hit (~ the jittered pixel), (x, y) for a miss, whose point is the unjittered far point
            qc = np.concatenate([x, np.ones((H, W, 1))], -1) @ np.linalg.inv(M).T
            sqc = np.where(qc[..., 3] > 0, qc[..., 3], 1.0)
            bx = np.where(hit, (qc[..., 0] / sqc + 1.0) / 2.0 * sw, xs)
            by = np.where(hit, (1.0 - qc[..., 1] / sqc) / 2.0 * sh, ys)
            f = np.float64(np.float32(camera.m_farClip))
            v = np.stack([(xs / sw * 2 - 1) * f, (1 - ys / sh * 2) * f, np.full_like(xs, f), np.full_like(xs, f)], -1)
            X = np.where(hit[..., None], xh, (v @ M.T)[..., :3])
            q = np.concatenate([X, np.ones((H, W, 1))], -1) @ prev["proj"].T
            seen = (q[..., 3] > 0) & (~hit | (qc[..., 3] > 0))
            sq = np.where(seen, q[..., 3], 1.0)
            fx = (q[..., 0] / sq + 1.0) / 2.0 * prev["screen"][0]
            fy = (1.0 - q[..., 1] / sq) / 2.0 * prev["screen"][1]
            rest = (cam_bytes == prev["cam"]) & ~moved
            m = np.where((seen & ~rest)[..., None], np.stack([fx - bx, fy - by], -1), 0.0)
            motion = np.where(known[..., None], m, 0.0)
            ok = known & (seen | rest) & ~rep
            hx, hy = xs + motion[..., 0], ys + motion[..., 1]
            valid = ok & (hx >= 0) & (hx <= W - 1) & (hy >= 0) & (hy <= H - 1)
            moving = ok & ~rest
            for h, lim in ((hx, W - 1), (hy, H - 1)):
                near |= moving & (_near(h, 0.0) | _near(h, float(lim)))
                near |= valid & ~rest & _near(h, np.floor(h) + 0.5)  # (the nearest tap; the resampling is continuous across integers)
            vx, vy = np.where(valid, hx, 0.0), np.where(valid, hy, 0.0)
            x0, y0 = np.floor(vx), np.floor(vy)
            tx, ty = vx - x0, vy - y0
            if p["flags"] & T.TAA_BILINEAR:
                offs = (0, 1)
                wx, wy = np.stack([1 - tx, tx], -1), np.stack([1 - ty, ty], -1)
            else:
                offs = (-1, 0, 1, 2)
                wx, wy = catmull_rom(tx), catmull_rom(ty)
            hist = np.zeros((H, W, 3))
            for r, oy in enumerate(offs):
                jy = np.clip(y0 + oy, 0, H - 1).astype(int)
                for k, ox in enumerate(offs):
                    jx = np.clip(x0 + ox, 0, W - 1).astype(int)
                    w = wy[..., r] * wx[..., k]
                    hist += w[..., None] * prev["hist"][jy, jx]
                    taint |= valid & (w != 0) & prev["taint"][jy, jx]
            valid &= np.isfinite(hist).all(-1)
            ny = np.clip(np.floor(vy + 0.5), 0, H - 1).astype(int)
            nx = np.clip(np.floor(vx + 0.5), 0, W - 1).astype(int)
            len_h = prev["length"][ny, nx]
            taint |= valid & prev["taint"][ny, nx]
            if not p["flags"] & T.TAA_NO_CLAMP:
                lo, hi = neighbourhood_box(c, np.float64(np.float32(p["gamma"])))
                hist = np.minimum(np.maximum(hist @ YCOCG.T, lo), hi) @ RGB.T
            length = np.where(valid, np.minimum(len_h + 1.0, MAX_LENGTH), 1.0)
            alpha = np.maximum(np.float64(np.float32(p["alpha_min"])), 1.0 / length)
            out = np.where(valid[..., None], hist + alpha[..., None] * (c - hist), c)
        taint |= near
        self.prev = {"shape": (H, W), "cam": cam_bytes, "proj": np.linalg.inv(M), "screen": (sw, sh), "models": list(models),
                     "hist": out, "length": length, "taint": taint}
        return {"out": out, "motion": motion, "length": length, "valid": valid, "near": near, "tainted": taint}
