"""CPU reference of the temporal upsampler (ff_taa_upscale): test infrastructure only.

TaaUpscaleRef.step is one call of include/firefly/ff_api.h's ff_taa_upscale in numpy, written from the steps there.  Steps 2 and 3
(where a high pixel looks in the low frame, the nearest low sample and the confidence k) are evaluated in float32 in the operator's
own operation order, so that both sides pick the same low sample and the same k; everything else is float64: the motion through
the G-buffer (taa_ref.TaaRef's, on the high grid), the history resampling, the clamp box over the low frame, the spatial estimate
and the blend.  It keeps the history between calls as the state does and reports TaaRef's `near` / `tainted` masks: pixels whose
validity bound or nearest-tap decision was within 1e-5 of its threshold, and every pixel whose history reads one of them.
"""
import numpy as np

from gpupathtracer_amd import types as T
from taa_ref import MAX_LENGTH, RGB, YCOCG, _near, catmull_rom, neighbourhood_box
from temporal_ref import ray_matrix

BLEND, HOLD, FIRST, SPATIAL = 0, 1, 2, 3  # step 6's four cases (`case` of step()'s result)


def _params(p):
    if isinstance(p, dict):
        return dict(p)
    return {f: (tuple(getattr(p, f)) if f == "lo_jitter" else getattr(p, f)) for f, _ in T.FfTaaUpscaleParams._fields_}


def look(n_hi, n_lo, jitter):
    """Steps 2 and 3 along one axis, in float32: (u, nearest low index i*, tent factor max(0, 1 - |u - i*| * s)) per high coordinate."""
    f32 = np.float32
    X = np.arange(n_hi, dtype=np.float32)
    u = (X * f32(n_lo)) / f32(n_hi) - f32(jitter)
    near = np.clip(np.floor(u + f32(0.5)), 0, n_lo - 1)
    d = u - near.astype(np.float32)
    s = f32(n_hi) / f32(n_lo)
    tent = np.maximum(f32(0.0), f32(1.0) - np.abs(d) * s)
    assert u.dtype == d.dtype == tent.dtype == np.float32
    return u, near.astype(np.int64), tent


def spatial_estimate(r, ids_lo, ids_hi, u, v, nearest):
    """Step 4 in float64: (c_up [H,W,3], fell [H,W] bool: the nearest low pixel was taken as it is)."""
    h, w = r.shape[:2]
    H, W = ids_hi.shape[:2]
    flu, flv = np.floor(u), np.floor(v)
    i0, j0 = flu.astype(np.int64), flv.astype(np.int64)
    fu, fv = (u - flu).astype(np.float64), (v - flv).astype(np.float64)
    bu, bv = {0: 1.0 - fu, 1: fu}, {0: 1.0 - fv, 1: fv}
    finite = np.isfinite(r).all(-1)

    def gather(taps, bilinear):
        acc, ws = np.zeros((H, W, 3)), np.zeros((H, W))
        for dj in taps:
            for di in taps:
                qi = np.broadcast_to(np.clip(i0 + di, 0, w - 1)[None, :], (H, W))
                qj = np.broadcast_to(np.clip(j0 + dj, 0, h - 1)[:, None], (H, W))
                b = bv[dj][:, None] * bu[di][None, :] if bilinear else np.ones((H, W))
                ok = finite[qj, qi] & (b > 0) & (ids_lo[qj, qi, 0] == ids_hi[..., 0]) & (ids_lo[qj, qi, 2] == ids_hi[..., 2])
                acc += np.where(ok[..., None], b[..., None] * np.where(finite[qj, qi][..., None], r[qj, qi], 0.0), 0.0)
                ws += np.where(ok, b, 0.0)
        return acc, ws

    acc2, ws2 = gather((0, 1), True)
    acc4, ws4 = gather((-1, 0, 1, 2), False)
    c = np.where((ws2 > 0)[..., None], acc2 / np.where(ws2 > 0, ws2, 1.0)[..., None], acc4 / np.where(ws4 > 0, ws4, 1.0)[..., None])
    fell = ~(ws2 > 0) & ~(ws4 > 0)
    return np.where(fell[..., None], nearest, c), fell


class TaaUpscaleRef:
    """ff_taa_upscale with a history of its own; step() is one call."""

    def __init__(self):
        self.reset()

    def reset(self):
        self.prev = None

    def step(self, radiance_lo, ids_lo, gbuffer_hi, camera, models, p, replaced=()):
        """radiance_lo [h,w,3] and ids_lo [h,w,3]: the low frame and ff_gbuffer's ids under p's lo_jitter; gbuffer_hi: ff_gbuffer's
        dict (position, ids) of `camera` at W x H, unjittered; models: temporal_ref.scene_models() of the scene as it is now; p: an
        FfTaaUpscaleParams or a dict of its fields; replaced: geometries whose mesh ff_update_mesh replaced since the last call.
        Returns a dict: out [H,W,3] float64, motion [H,W,2], length [H,W], valid, near, tainted [H,W] bool, k [H,W] float32,
        case [H,W] (BLEND, HOLD, FIRST, SPATIAL), fell [H,W] bool (c_up is the nearest low pixel as it is)."""
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            return self._step(radiance_lo, ids_lo, gbuffer_hi, camera, models, p, replaced)

    def _step(self, radiance_lo, ids_lo, gbuffer, camera, models, p, replaced):
        p = _params(p)
        r = np.asarray(radiance_lo, dtype=np.float32).astype(np.float64)
        ids_lo = np.asarray(ids_lo)
        h, w = r.shape[:2]
        ids = np.asarray(gbuffer["ids"])
        geom = ids[..., 0]
        H, W = geom.shape
        hit = geom >= 0
        x = np.asarray(gbuffer["position"], dtype=np.float32).astype(np.float64)
        ys, xs = np.mgrid[0:H, 0:W].astype(np.float64)
        M = ray_matrix(camera)
        sw, sh = np.float64(np.float32(camera.m_screenWidth)), np.float64(np.float32(camera.m_screenHeight))
        motion = np.zeros((H, W, 2))
        valid = np.zeros((H, W), bool)
        near = np.zeros((H, W), bool)
        taint = np.zeros((H, W), bool)
        hist = np.zeros((H, W, 3))
        len_h = np.zeros((H, W))
        cam_bytes = bytes(camera)
        prev = self.prev
        # 1. motion, history, length: TaaRef's on the W x H grid
        if prev is not None and prev["shape"] == (H, W, h, w):
            moved = np.zeros((H, W), bool)
            rep = np.zeros((H, W), bool)
            known = ~hit | (geom < len(models))
            xh = x.copy()
            for g, (mod, inv) in enumerate(models):
                on = hit & (geom == g)
                if g in replaced:
                    rep |= on
                pm = prev["models"][g][0] if g < len(prev["models"]) else None
                if pm is None or np.array_equal(pm[:3], mod[:3]):
                    continue
                A = pm @ inv
                moved |= on
                xh[on] = x[on] @ A[:3, :3].T + A[:3, 3]
            qc = np.concatenate([x, np.ones((H, W, 1))], -1) @ np.linalg.inv(M).T
            sqc = np.where(qc[..., 3] > 0, qc[..., 3], 1.0)
            bx = np.where(hit, (qc[..., 0] / sqc + 1.0) / 2.0 * sw, xs)
            by = np.where(hit, (1.0 - qc[..., 1] / sqc) / 2.0 * sh, ys)
            f = np.float64(np.float32(camera.m_farClip))
            far = np.stack([(xs / sw * 2 - 1) * f, (1 - ys / sh * 2) * f, np.full_like(xs, f), np.full_like(xs, f)], -1)
            X = np.where(hit[..., None], xh, (far @ M.T)[..., :3])
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
            for hh, lim in ((hx, W - 1), (hy, H - 1)):
                near |= moving & (_near(hh, 0.0) | _near(hh, float(lim)))
                near |= valid & ~rest & _near(hh, np.floor(hh) + 0.5)
            vx, vy = np.where(valid, hx, 0.0), np.where(valid, hy, 0.0)
            x0, y0 = np.floor(vx), np.floor(vy)
            tx, ty = vx - x0, vy - y0
            if p["flags"] & T.TAA_BILINEAR:
                offs = (0, 1)
                wx, wy = np.stack([1 - tx, tx], -1), np.stack([1 - ty, ty], -1)
            else:
                offs = (-1, 0, 1, 2)
                wx, wy = catmull_rom(tx), catmull_rom(ty)
            for rr, oy in enumerate(offs):
                jy = np.clip(y0 + oy, 0, H - 1).astype(int)
                for cc, ox in enumerate(offs):
                    jx = np.clip(x0 + ox, 0, W - 1).astype(int)
                    wt = wy[..., rr] * wx[..., cc]
                    hist += wt[..., None] * prev["hist"][jy, jx]
                    taint |= valid & (wt != 0) & prev["taint"][jy, jx]
            valid &= np.isfinite(hist).all(-1)
            ny = np.clip(np.floor(vy + 0.5), 0, H - 1).astype(int)
            nx = np.clip(np.floor(vx + 0.5), 0, W - 1).astype(int)
            len_h = np.where(valid, prev["length"][ny, nx], 0.0)
            taint |= valid & prev["taint"][ny, nx]
        # 2, 3. the nearest low sample and the confidence, in float32
        u, i_s, tent_x = look(W, w, p["lo_jitter"][0])
        v, j_s, tent_y = look(H, h, p["lo_jitter"][1])
        k = tent_x[None, :] * tent_y[:, None]
        assert k.dtype == np.float32
        I, J = np.broadcast_to(i_s[None, :], (H, W)), np.broadcast_to(j_s[:, None], (H, W))
        c = r[J, I]
        same = (ids_lo[J, I, 0] == ids[..., 0]) & (ids_lo[J, I, 2] == ids[..., 2])
        k = np.where(same & np.isfinite(c).all(-1), k, np.float32(0.0)).astype(np.float32)
        kd = k.astype(np.float64)
        # 4. spatial estimate
        c_up, fell = spatial_estimate(r, ids_lo, ids, u, v, c)
        # 5. clamp
        clamped = hist
        if not p["flags"] & T.TAA_NO_CLAMP:
            lo, hi = neighbourhood_box(r, np.float64(np.float32(p["gamma"])))
            box = np.minimum(np.maximum(hist @ YCOCG.T, lo[J, I]), hi[J, I]) @ RGB.T
            clamped = np.where(np.isfinite(box), box, hist)  # (no finite sample: nothing is clamped; only read where k > 0)
        # 6. blend
        wsum = np.minimum(len_h + kd, MAX_LENGTH)
        alpha = np.maximum(np.float64(np.float32(p["alpha_min"])) * kd, kd / np.where(wsum > 0, wsum, 1.0))
        cz = np.where(np.isfinite(c), c, 0.0)  # (c is only blended where k > 0, where it is finite)
        case = np.where(valid & (wsum > 0), np.where(kd > 0, BLEND, HOLD), np.where(~valid & (kd > 0), FIRST, SPATIAL))
        out = np.where((case == BLEND)[..., None], clamped + alpha[..., None] * (cz - clamped),
                       np.where((case == HOLD)[..., None], hist, np.where((case == FIRST)[..., None], cz, c_up)))
        length = np.where(case == BLEND, wsum, np.where(case == HOLD, len_h, np.where(case == FIRST, kd, 0.0)))
        taint |= near
        self.prev = {"shape": (H, W, h, w), "cam": cam_bytes, "proj": np.linalg.inv(M), "screen": (sw, sh), "models": list(models),
                     "hist": out, "length": length, "taint": taint}
        return {"out": out, "motion": motion, "length": length, "valid": valid, "near": near, "tainted": taint, "k": k, "case": case,
                "fell": fell}
