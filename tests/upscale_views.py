"""A scene-free G-buffer for the ff_upscale tests: test infrastructure only.

view(w, h, jitter) is one fixed synthetic picture, parametrised in [0,1]^2, so a low view and a high view of any two sizes and
aspects show the same thing; noisy_radiance(gb, seed) is a seeded radiance over it.  EDGE_PAIRS, EDGE_FLAGS, EDGE_JITTERS and
EDGE_SIGMAS are the edge cases the host twin (test_upscale_host.py) and the kernel (test_gpu_upscale_edges.py) are both held to.
"""
import numpy as np

from gpupathtracer_amd import types as T
from gbuffer_ref import filterable

# (low, high) sizes: a low image of one pixel, one row and one column (every tap clamps); factor 8, the largest the API takes;
# factor 1; ratios that differ along x and y; high images narrower than a 64-wide wave row and lower than a 4-row workgroup, and
# one partial workgroup past each
EDGE_PAIRS = [((1, 1), (1, 1)), ((1, 1), (8, 8)), ((1, 5), (3, 37)), ((5, 1), (37, 1)), ((2, 3), (16, 24)), ((7, 5), (7, 5)),
              ((9, 7), (65, 35)), ((33, 17), (65, 17)), ((8, 33), (64, 257)), ((21, 12), (161, 91)), ((63, 4), (64, 5)),
              ((129, 3), (257, 5))]
EDGE_FLAGS = [0, T.DENOISE_SAME_GEOMETRY, T.DENOISE_SAME_GEOMETRY | T.DENOISE_DEMODULATE_ALBEDO]
EDGE_JITTERS = [((0.0, 0.0), (0.0, 0.0)), ((0.5, 0.25), (0.0, 0.0)), ((0.9375, 0.0625), (0.25, 0.75))]  # (lo, hi)
EDGE_SIGMAS = [(0.1, 0.1), (0.0125, 0.1), (0.8, 0.1), (0.1, 0.0125), (0.1, 0.8)]  # (normal, plane)
SCALING_EXPONENT = 20  # out(rad * 2^-+20) == out(rad) * 2^-+20: decided by the host twin (test_upscale_host.py), then asked of the kernel
ZERO_NORMAL_BOX = (0.4, 0.62, 0.2, 0.38)  # s0, s1, t0, t1: filterable pixels of both planes, across the edge s = 0.55


def pair_id(pair):
    (w, h), (W, H) = pair
    return f"{w}x{h}-{W}x{H}"


def view(w, h, jitter=(0.0, 0.0), zero_normal=False):
    """The G-buffer of one fixed synthetic view at w x h under a pixel jitter: pixel (x, y) looks at s = (x + jx) / w,
    t = (y + jy) / h.  Two planes meeting at the edge s = 0.55 (the left one with a checker albedo of 48 x 27 squares, the right one
    tilted, its normal not unit length and its green albedo 0 in a band), a disc with a sphere's normals, a band of misses on top,
    an emitter and a mirror.  zero_normal: the pixels of ZERO_NORMAL_BOX, all filterable, get the normal (0, 0, 0)."""
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    s, t = (xx + jitter[0]) / w, (yy + jitter[1]) / h
    ids = np.zeros((h, w, 3), np.int32)
    ids[..., 1] = -1
    ids[..., 2] = T.BXDF_DIFFUSE
    pos = np.stack([s, t, np.zeros_like(s)], -1)
    nrm = np.zeros((h, w, 3)) + np.array([0.0, 0.0, 1.0])
    checker = ((np.floor(s * 48) + np.floor(t * 27)) % 2 == 0)[..., None]
    alb = np.where(checker, np.array([0.8, 0.6, 0.4]), np.array([0.2, 0.3, 0.5]))
    right = s >= 0.55
    ids[right, 0] = 1
    pos[right, 2] = (s[right] - 0.55) * 0.8
    nrm[right] = np.array([-0.8, 0.0, 1.0]) * 1.7
    alb[right] = np.array([0.7, 0.5, 0.6])
    alb[right & (t > 0.7), 1] = 0.0
    dx, dy = s - 0.3, t - 0.55
    disc = dx * dx + dy * dy < 0.15 ** 2
    ids[disc, 0] = 2
    nz = np.sqrt(np.maximum(0.15 ** 2 - dx * dx - dy * dy, 0.0))
    sphere_n = np.stack([dx, dy, nz], -1) / 0.15
    nrm[disc] = sphere_n[disc]
    pos[disc] = (np.array([0.3, 0.55, 0.0]) + 0.15 * sphere_n)[disc]
    alb[disc] = np.array([0.9, 0.9, 0.2])
    for geom, kind, box, colour in ((3, T.BXDF_EMITTER, (0.62, 0.8, 0.3, 0.5), (5.0, 5.0, 5.0)), (4, T.BXDF_MIRROR, (0.1, 0.3, 0.15, 0.3), (0.9, 0.9, 0.9))):
        m = (s >= box[0]) & (s < box[1]) & (t >= box[2]) & (t < box[3])
        ids[m, 0] = geom
        ids[m, 2] = kind
        alb[m] = colour
    miss = t < 0.12
    ids[miss] = -1
    pos[miss] = 0.0
    nrm[miss] = 0.0
    alb[miss] = 0.0
    if zero_normal:
        s0, s1, t0, t1 = ZERO_NORMAL_BOX
        nrm[(s >= s0) & (s < s1) & (t >= t0) & (t < t1) & filterable(ids)] = 0.0
    return {"ids": ids, "position": pos.astype(np.float32), "normal": nrm.astype(np.float32), "albedo": alb.astype(np.float32)}


def noisy_radiance(gb, seed=7):
    """Smooth light times the albedo times seeded noise on the filterable pixels; sky, emitter and mirror colours elsewhere."""
    rng = np.random.default_rng(seed)
    h, w = gb["ids"].shape[:2]
    yy, xx = np.mgrid[0:h, 0:w]
    light = np.stack([0.6 + 0.3 * np.sin(xx * 9.0 / w), 0.5 + 0.2 * np.cos(yy * 7.0 / h), 0.4 + 0.3 * xx / w], -1)
    rad = light * np.where(gb["albedo"] > 0, gb["albedo"], 0.3) * rng.uniform(0.5, 1.5, size=(h, w, 3))
    rad = np.where(filterable(gb["ids"])[..., None], rad, gb["albedo"] * rng.uniform(0.9, 1.1, size=(h, w, 3)) + 0.05 * yy[..., None] / h)
    return rad.astype(np.float32)


def zero_normal_patch(gb):
    """[h,w] bool: the filterable pixels whose normal is (0, 0, 0)."""
    return filterable(gb["ids"]) & ~gb["normal"].any(-1)
