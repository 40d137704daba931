"""CPU reference of the temporal denoiser (ff_denoise_temporal): test infrastructure only.

TemporalRef.step is one call of include/firefly/ff_api.h's ff_denoise_temporal in float64 numpy, written from the formulas there:
reprojection through the previous camera and the geometries' rigid motion, tap validity, accumulation of colour and luminance
moments, the variance estimate, the variance-guided à-trous passes, the colour feedback and the remodulation.  It keeps the
history between calls as the state does.  Besides the output it reports, per pixel, whether any validity test or floor decision
was within 1e-5 (relative) of its threshold: such pixels may legitimately decide the other way in float32.  `tainted` adds every
pixel whose result reads one of them with a nonzero weight: a tap of the history (across calls), of the spatial variance or of
a pass.

Non-finite input follows ff_api.h: a tap whose stored colour or moments are not all finite is no history, a tap that weighs 0
adds nothing (not 0 * its value), and max(0, v) is fmax (a NaN v gives 0), as the kernels compute it.
"""
import ctypes as C

import numpy as np

from gpupathtracer_amd import types as T
from gbuffer_ref import B3, MAX_EXPONENT, PLANE_EPS, _shift, filterable

LUM = np.array([0.2126, 0.7152, 0.0722])
LUM_EPS = 1e-30
MIN_HISTORY_WEIGHT = 1e-3
NEAR = 1e-5


def luminance(c):
    return c @ LUM


def ray_matrix(camera):
    """ff_camera_ray_matrix(camera) as a float64 4x4 (row, column) matrix of the float32 values."""
    from gpupathtracer_amd import lib
    m = T.FfMat4()
    lib.load().ff_camera_ray_matrix(C.byref(camera), C.byref(m))
    return np.array(m.m[:], dtype=np.float32).astype(np.float64).reshape(4, 4).T


def scene_models(scene):
    """Per caller geometry index: the float32 (model, inverse model) matrices as float64 4x4 (row, column) arrays."""
    out = []
    for i in range(len(scene)):
        g = scene.geometries[i]
        mod = np.array(g.m_modelMatrix.m[:], dtype=np.float32).astype(np.float64).reshape(4, 4).T
        inv = np.array(g.m_inverseModelMatrix.m[:], dtype=np.float32).astype(np.float64).reshape(4, 4).T
        out.append((mod, inv))
    return out


def unit(v):
    ln = np.sqrt((v * v).sum(-1, keepdims=True))
    return np.where(ln > 0, v / np.where(ln > 0, ln, 1.0), 0.0)


def _params(tp):
    names = [f for f, _ in T.FfTemporalParams._fields_]
    return {f: getattr(tp, f) for f in names} if not isinstance(tp, dict) else dict(tp)


class TemporalRef:
    """ff_denoise_temporal with a history of its own; step() is one call."""

    def __init__(self):
        self.reset()

    def reset(self):
        self.prev = None

    def step(self, radiance, gbuffer, camera, models, tp, replaced=()):
        """radiance [H,W,3]; gbuffer: ff_gbuffer's dict for `camera`; models: scene_models() of the scene as it is now; tp: an
        FfTemporalParams or a dict of its fields; replaced: geometries whose mesh ff_update_mesh replaced since the last call.
        Returns a dict: out [H,W,3] float64, motion [H,W,2], length [H,W], near [H,W] bool, tainted [H,W] bool."""
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            return self._step(radiance, gbuffer, camera, models, tp, replaced)

    def _step(self, radiance, gbuffer, camera, models, tp, replaced):
        p = _params(tp)
        rad = np.asarray(radiance, dtype=np.float64)
        H, W = rad.shape[:2]
        ids = np.asarray(gbuffer["ids"])
        geom = ids[..., 0]
        hit = geom >= 0
        filt = filterable(ids)
        cls = np.where(filt, geom, -1)
        n = unit(np.asarray(gbuffer["normal"], dtype=np.float32).astype(np.float64))
        x = np.asarray(gbuffer["position"], dtype=np.float32).astype(np.float64)
        demod = bool(p["flags"] & T.DENOISE_DEMODULATE_ALBEDO)
        same_geometry = bool(p["flags"] & T.DENOISE_SAME_GEOMETRY)
        c = rad.copy()
        if demod:
            a = np.asarray(gbuffer["albedo"], dtype=np.float32).astype(np.float64)
            div = (a > 0) & filt[..., None]
            c[div] = rad[div] / a[div]
        l = luminance(c)
        ys, xs = np.mgrid[0:H, 0:W].astype(np.float64)
        motion = np.zeros((H, W, 2))
        near = np.zeros((H, W), bool)
        inherited = np.zeros((H, W), bool)  # a history tap that counts is tainted
        wsum = np.zeros((H, W))
        hc = np.zeros((H, W, 3))
        hm = np.zeros((H, W, 3))  # m1, m2, len
        cam_bytes = bytes(camera)
        prev = self.prev
        if prev is not None and prev["shape"] == (H, W):
            moved = np.zeros((H, W), bool)
            xh, nh = x.copy(), n.copy()
            rep = np.zeros((H, W), bool)
            for k, (mod, inv) in enumerate(models):
                on = hit & (geom == k)
                if k in replaced:
                    rep |= on
                pm = prev["models"][k][0] if k < len(prev["models"]) else None
                if pm is None or np.array_equal(pm[:3], mod[:3]):
                    continue
                A = pm @ inv
                A[3] = (0, 0, 0, 1)
                N = np.linalg.inv(A[:3, :3]).T
                moved |= on
                xh[on] = x[on] @ A[:3, :3].T + A[:3, 3]
                nh[on] = unit(n[on] @ N.T)
            q = np.concatenate([xh, np.ones((H, W, 1))], -1) @ prev["proj"].T
            qw = q[..., 3]
            seen = qw > 0
            sqw = np.where(seen, qw, 1.0)
            fx = (q[..., 0] / sqw + 1.0) / 2.0 * prev["screen"][0]
            fy = (1.0 - q[..., 1] / sqw) / 2.0 * prev["screen"][1]
            rest = (cam_bytes == prev["cam"]) & ~moved
            fx = np.where(rest, xs, fx)
            fy = np.where(rest, ys, fy)
            seen |= rest
            known = geom < len(models)  # (ids that name no geometry of the scene have no history and no motion)
            motion = np.where((hit & known & seen)[..., None], np.stack([fx - xs, fy - ys], -1), 0.0)
            cand = filt & known & seen & ~rep & (fx > -1) & (fx < W) & (fy > -1) & (fy < H)
            cfx, cfy = np.where(cand, fx, 0.0), np.where(cand, fy, 0.0)
            x0, y0 = np.floor(cfx), np.floor(cfy)
            ax, ay = cfx - x0, cfy - y0
            for f in (cfx, cfy):
                near |= cand & ~rest & (np.abs(f - np.round(f)) <= NEAR * np.maximum(1.0, np.abs(f)))
            lim = p["reuse_plane"] * np.sqrt(((xh - prev["eye"]) ** 2).sum(-1))
            rn = p["reuse_normal"]
            for t in range(4):
                tx, ty = x0 + (t & 1), y0 + (t >> 1)
                wt = (ax if t & 1 else 1.0 - ax) * (ay if t >> 1 else 1.0 - ay)
                inside = cand & (tx >= 0) & (tx < W) & (ty >= 0) & (ty < H) & (wt > 0)
                jx = np.clip(tx, 0, W - 1).astype(int)
                jy = np.clip(ty, 0, H - 1).astype(int)
                same = inside & (prev["cls"][jy, jx] == cls)
                dn = (nh * prev["n"][jy, jx]).sum(-1)
                pd = np.abs((nh * (prev["x"][jy, jx] - xh)).sum(-1))
                finite = np.isfinite(prev["col"][jy, jx]).all(-1) & np.isfinite(prev["mom"][jy, jx]).all(-1)
                ok = same & (dn >= rn) & (pd <= lim) & finite
                # (pd's float32 error is of the order of the coordinates' rounding, so the band around lim is at least 1e-7 of the
                # distance: with reuse_plane 0, lim = 0 and a pd of 0 in one precision may be a few ulps in the other)
                plane_band = NEAR * np.maximum(lim, 1e-2 * np.sqrt(((xh - prev["eye"]) ** 2).sum(-1)))
                near |= same & ((np.abs(dn - rn) <= NEAR * max(abs(rn), 1e-30)) | (np.abs(pd - lim) <= plane_band))
                w = np.where(ok, wt, 0.0)
                inherited |= ok & prev["taint"][jy, jx]
                wsum += w
                hc += np.where(ok[..., None], w[..., None] * prev["col"][jy, jx], 0.0)
                hm += np.where(ok[..., None], w[..., None] * prev["mom"][jy, jx], 0.0)
            near |= (wsum > 0) & (np.abs(wsum - MIN_HISTORY_WEIGHT) <= NEAR * MIN_HISTORY_WEIGHT)
        have = wsum >= MIN_HISTORY_WEIGHT
        sw = np.where(have, wsum, 1.0)[..., None]
        hc, hm = hc / sw, hm / sw
        length = np.where(have, hm[..., 2] + 1.0, 1.0)
        alpha = 1.0 / np.minimum(length, p["max_history"])
        acc = np.where(have[..., None], hc + alpha[..., None] * (c - hc), c)
        m1 = np.where(have, hm[..., 0] + alpha * (l - hm[..., 0]), l)
        m2 = np.where(have, hm[..., 1] + alpha * (l * l - hm[..., 1]), l * l)
        length = np.where(filt, length, 0.0)
        m1, m2 = np.where(filt, m1, 0.0), np.where(filt, m2, 0.0)
        col_hist = acc.copy()
        c = acc
        taint = near | inherited
        if p["iterations"] > 0:
            var = np.fmax(0.0, m2 - m1 * m1)
            short = filt & (length < p["variance_history"])
            if short.any():
                inv_sn = 1.0 / np.float64(np.float32(p["sigma_normal"]))
                sp2 = np.float64(np.float32(p["sigma_plane"])) ** 2
                s1, s2, ws = m1.copy(), m2.copy(), np.ones((H, W))
                for dy in range(-3, 4):
                    for dx in range(-3, 4):
                        if dx == 0 and dy == 0:
                            continue
                        qcls = _shift(cls, dy, dx, -1)
                        ok = filt & (qcls == cls)
                        a_n = (1.0 - (n * _shift(n, dy, dx, 0.0)).sum(-1)) * inv_sn
                        v = _shift(x, dy, dx, 0.0) - x
                        pd = (n * v).sum(-1)
                        a_x = pd * pd / (sp2 * (v * v).sum(-1) + PLANE_EPS)
                        e = a_n + a_x
                        take = ok & (e <= MAX_EXPONENT)
                        w = np.where(take, np.exp(-np.minimum(e, MAX_EXPONENT)), 0.0)
                        ws += w
                        taint = taint | (short & (w > 0) & _shift(near | inherited, dy, dx, False))
                        s1 += np.where(take, w * _shift(m1, dy, dx, 0.0), 0.0)
                        s2 += np.where(take, w * _shift(m2, dy, dx, 0.0), 0.0)
                mu1, mu2 = s1 / ws, s2 / ws
                spatial = np.fmax(0.0, mu2 - mu1 * mu1) * 4.0 / np.where(length > 0, length, 1.0)
                var = np.where(short, spatial, var)
            var = np.where(filt, var, 0.0)
            c, var, fed, taint = atrous_passes(c, var, n, x, cls, filt, p, same_geometry, taint)
            if p["feedback_pass"] >= 0:
                col_hist = fed
        out = c
        if demod:
            out = np.where(div, c * a, c)
        out = np.where(filt[..., None], out, rad)
        self.prev = {"shape": (H, W), "cam": cam_bytes, "proj": np.linalg.inv(ray_matrix(camera)),
                     "eye": np.array([camera.m_position.x, camera.m_position.y, camera.m_position.z], dtype=np.float32).astype(np.float64),
                     "screen": (np.float64(np.float32(camera.m_screenWidth)), np.float64(np.float32(camera.m_screenHeight))),
                     "models": [m for m in models], "cls": cls, "n": n, "x": x, "col": col_hist, "mom": np.stack([m1, m2, length], -1), "taint": taint}
        return {"out": out, "motion": motion, "length": length, "near": near, "tainted": taint}


def atrous_passes(c, var, n, x, cls, filt, p, same_geometry, taint):
    """The variance-guided passes; returns (colour, variance, colour after pass feedback_pass, taint spread by the taps)."""
    H, W = cls.shape
    inv_sn = 1.0 / np.float64(np.float32(p["sigma_normal"]))
    sp2 = np.float64(np.float32(p["sigma_plane"])) ** 2
    sl = np.float64(np.float32(p["sigma_luminance"]))
    fed = None
    h0 = B3[2] * B3[2]
    for i in range(p["iterations"]):
        step = 1 << i
        ksum, gsum = np.full((H, W), 4.0), 4.0 * var
        spread = taint.copy()
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                if dx == 0 and dy == 0:
                    continue
                qcls = _shift(cls, dy, dx, -1)
                ok = qcls >= 0
                if same_geometry:
                    ok &= qcls == cls
                k = (2 - abs(dx)) * (2 - abs(dy))
                ksum += k * ok
                spread |= filt & ok & _shift(taint, dy, dx, False)
                gsum += np.where(ok, k * _shift(var, dy, dx, 0.0), 0.0)
        den = sl * np.sqrt(gsum / ksum) + LUM_EPS
        lp = luminance(c)
        wsum, vsum, acc = np.full((H, W), h0), h0 * h0 * var, np.zeros_like(c)
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                if dx == 0 and dy == 0:
                    continue
                oy, ox = dy * step, dx * step
                qcls = _shift(cls, oy, ox, -1)
                ok = filt & (qcls >= 0)
                if same_geometry:
                    ok &= qcls == cls
                cq = _shift(c, oy, ox, 0.0)
                a_l = np.abs(lp - luminance(cq)) / den
                a_n = (1.0 - (n * _shift(n, oy, ox, 0.0)).sum(-1)) * inv_sn
                v = _shift(x, oy, ox, 0.0) - x
                pd = (n * v).sum(-1)
                a_x = pd * pd / (sp2 * (v * v).sum(-1) + PLANE_EPS)
                e = a_l + a_n + a_x
                take = ok & (e <= MAX_EXPONENT)
                w = np.where(take, B3[dx + 2] * B3[dy + 2] * np.exp(-np.minimum(e, MAX_EXPONENT)), 0.0)
                wsum += w
                spread |= (w > 0) & _shift(taint, oy, ox, False)
                vsum += np.where(take, w * w * _shift(var, oy, ox, 0.0), 0.0)
                acc += np.where(take[..., None], w[..., None] * (c - cq), 0.0)
        c = np.where(filt[..., None], c - acc / wsum[..., None], c)
        var = np.where(filt, vsum / (wsum * wsum), var)
        taint = spread
        if i == p["feedback_pass"]:
            fed = c.copy()
    return c, var, fed, taint
