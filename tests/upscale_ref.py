"""CPU reference for ff_upscale: test infrastructure only.

upscale_ref: the operator of include/firefly/ff_api.h (ff_upscale) in float64 numpy, written from the steps there.  The tap
coordinates i0, j0 and the fractions fu, fv come from the float32 expression the kernel evaluates, so that a floor cannot differ;
everything after that is float64, with the mean as the plain sum w c_q / sum w.

bilinear_ref: plain bilinear upsampling of the low image on the same grid (what the guided operator is compared against).
"""
import numpy as np

from gpupathtracer_amd import types as T
from gbuffer_ref import filterable

PLANE_EPS = 1e-30
MAX_EXPONENT = 30.0  # taps with a_n + a_x above it weigh 0

STEP_2X2, STEP_4X4, STEP_FALLBACK = 2, 3, 4  # which rule produced a pixel (upscale_ref's `steps`)


def low_coordinates(n_hi, n_lo, hi_jitter, lo_jitter):
    """(i0 int, f float32, u float32) of the high coordinates 0 .. n_hi-1 along one axis: u = ((X + J) * n_lo) / n_hi - j in float32."""
    f32 = np.float32
    X = np.arange(n_hi, dtype=np.float32)
    u = ((X + f32(hi_jitter)) * f32(n_lo)) / f32(n_hi) - f32(lo_jitter)
    assert u.dtype == np.float32
    fl = np.floor(u)
    return fl.astype(np.int64), (u - fl).astype(np.float32), u


def _unit(n):
    n = np.asarray(n, dtype=np.float64)
    ln = np.sqrt((n * n).sum(-1, keepdims=True))
    return np.where(ln > 0, n / np.where(ln > 0, ln, 1.0), 0.0)


def upscale_ref(radiance_lo, gbuffer_lo, gbuffer_hi, sigma_normal=0.1, sigma_plane=0.1,
                flags=T.DENOISE_SAME_GEOMETRY | T.DENOISE_DEMODULATE_ALBEDO, lo_jitter=(0.0, 0.0), hi_jitter=(0.0, 0.0), rows=None):
    """ff_upscale in float64 -> (radiance [H,W,3] float64, steps [H,W] int: STEP_2X2, STEP_4X4 or STEP_FALLBACK).  rows = (Y0, Y1):
    the high rows Y0 .. Y1-1 only ([Y1-Y0,W,...]: a large image is compared a band at a time)."""
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        return _upscale_ref(radiance_lo, gbuffer_lo, gbuffer_hi, sigma_normal, sigma_plane, flags, lo_jitter, hi_jitter, rows)


def _upscale_ref(radiance_lo, gl, gh, sigma_normal, sigma_plane, flags, lo_jitter, hi_jitter, rows=None):
    r = np.asarray(radiance_lo, dtype=np.float64)
    h, w = r.shape[:2]
    full_H = np.shape(gh["ids"])[0]
    Y0, Y1 = rows if rows is not None else (0, full_H)
    gh = {k: np.asarray(gh[k])[Y0:Y1] for k in ("ids", "position", "normal", "albedo") if k in gh}
    ids_P = gh["ids"]
    H, W = ids_P.shape[:2]
    ids_lo = np.asarray(gl["ids"])
    same = bool(flags & T.DENOISE_SAME_GEOMETRY)
    demod = bool(flags & T.DENOISE_DEMODULATE_ALBEDO)
    sn = float(np.float32(sigma_normal))
    sp2 = float(np.float32(sigma_plane) * np.float32(sigma_plane))  # (the library squares it in float32)
    i0, fu, u = low_coordinates(W, w, hi_jitter[0], lo_jitter[0])
    j0, fv, v = (c[Y0:Y1] for c in low_coordinates(full_H, h, hi_jitter[1], lo_jitter[1]))
    I0, J0 = np.broadcast_to(i0[None, :], (H, W)), np.broadcast_to(j0[:, None], (H, W))
    bu = {0: 1.0 - fu.astype(np.float64), 1: fu.astype(np.float64)}
    bv = {0: 1.0 - fv.astype(np.float64), 1: fv.astype(np.float64)}
    filt_P = filterable(ids_P)
    filt_lo = filterable(ids_lo)
    finite_lo = np.isfinite(r).all(-1)
    x_P = np.asarray(gh["position"], dtype=np.float64)
    n_P = _unit(gh["normal"])
    x_lo = np.asarray(gl["position"], dtype=np.float64)
    n_lo = _unit(gl["normal"])
    a_P = np.asarray(gh["albedo"], dtype=np.float64) if demod else np.zeros((H, W, 3))
    a_lo = np.asarray(gl["albedo"], dtype=np.float64) if demod else np.ones((h, w, 3))
    divide = (a_P > 0) & filt_P[..., None] if demod else np.zeros((H, W, 3), bool)

    def gather(taps, bilinear):
        """(sum w c [H,W,3], sum w [H,W]) over `taps` (offsets) for the filterable rule and for the other rule."""
        acc_f, ws_f = np.zeros((H, W, 3)), np.zeros((H, W))
        acc_o, ws_o = np.zeros((H, W, 3)), np.zeros((H, W))
        for dj in taps:
            for di in taps:
                qi, qj = np.clip(I0 + di, 0, w - 1), np.clip(J0 + dj, 0, h - 1)
                b = bu[di][None, :] * bv[dj][:, None] if bilinear else np.ones((H, W))
                rq = r[qj, qi]
                ok = finite_lo[qj, qi] & (b > 0)
                # P filterable
                okf = ok & filt_P & filt_lo[qj, qi]
                if same:
                    okf &= ids_lo[qj, qi, 0] == ids_P[..., 0]
                aq = a_lo[qj, qi]
                if demod:
                    okf &= (~(a_P > 0) | (aq > 0)).all(-1)
                a_n = (1.0 - (n_P * n_lo[qj, qi]).sum(-1)) / sn
                d = x_lo[qj, qi] - x_P
                pd = (n_P * d).sum(-1)
                a_x = pd * pd / (sp2 * (d * d).sum(-1) + PLANE_EPS)
                e = a_n + a_x
                okf &= e <= MAX_EXPONENT
                wq = np.where(okf, b * np.exp(-np.minimum(e, MAX_EXPONENT)), 0.0)
                cq = np.where(divide, rq / np.where(aq > 0, aq, 1.0), rq)
                acc_f += np.where(okf[..., None], wq[..., None] * cq, 0.0)
                ws_f += wq
                # P not filterable
                oko = ok & ~filt_P & (ids_lo[qj, qi, 0] == ids_P[..., 0]) & (ids_lo[qj, qi, 2] == ids_P[..., 2])
                wo = np.where(oko, b, 0.0)
                acc_o += np.where(oko[..., None], wo[..., None] * rq, 0.0)
                ws_o += wo
        acc = np.where(filt_P[..., None], acc_f, acc_o)
        ws = np.where(filt_P, ws_f, ws_o)
        return acc, ws

    acc2, ws2 = gather((0, 1), True)
    acc4, ws4 = gather((-1, 0, 1, 2), False)
    steps = np.where(ws2 > 0, STEP_2X2, np.where(ws4 > 0, STEP_4X4, STEP_FALLBACK))
    c = np.where((ws2 > 0)[..., None], acc2 / np.where(ws2 > 0, ws2, 1.0)[..., None], acc4 / np.where(ws4 > 0, ws4, 1.0)[..., None])
    c = np.where(divide, c * a_P, c)
    ni = np.clip(np.floor(u + np.float32(0.5)).astype(np.int64), 0, w - 1)
    nj = np.clip(np.floor(v + np.float32(0.5)).astype(np.int64), 0, h - 1)
    nearest = r[nj[:, None], ni[None, :]]
    return np.where((steps == STEP_FALLBACK)[..., None], nearest, c), steps


def bilinear_ref(radiance_lo, H, W, lo_jitter=(0.0, 0.0), hi_jitter=(0.0, 0.0)):
    """Plain bilinear upsampling of radiance_lo [h,w,3] to [H,W,3] (float64) on ff_upscale's grid, taps clamped into the image."""
    r = np.asarray(radiance_lo, dtype=np.float64)
    h, w = r.shape[:2]
    i0, fu, _ = low_coordinates(W, w, hi_jitter[0], lo_jitter[0])
    j0, fv, _ = low_coordinates(H, h, hi_jitter[1], lo_jitter[1])
    out = np.zeros((H, W, 3))
    for dj, bj in ((0, 1.0 - fv.astype(np.float64)), (1, fv.astype(np.float64))):
        for di, bi in ((0, 1.0 - fu.astype(np.float64)), (1, fu.astype(np.float64))):
            qi, qj = np.clip(i0 + di, 0, w - 1), np.clip(j0 + dj, 0, h - 1)
            out += (bj[:, None] * bi[None, :])[..., None] * r[qj[:, None], qi[None, :]]
    return out
