"""Shared inputs of the ff_interpolate tests (test_interpolate_host.py, test_gpu_interpolate.py): test infrastructure only.

view(w, h, pose) casts the primary rays of a real FfCamera against one fixed synthetic scene - no scene upload, no tracer - and
gives ff_gbuffer's position and ids planes: two walls meeting at an edge (the right one tilted towards the viewer), a disc in front
of them, a band of misses above the walls, an emitter and a mirror patch, and a small tag on the left wall right above the disc's
rim.  The three poses are a few pixels of parallax apart; the mid pose lies ABOVE the line from A to B, so the disc uncovers wall
that A sees and B does not, the other way round, a sliver that neither sees - and the tag, which only the mid pose sees at all.
"""
import numpy as np

from gpupathtracer_amd import scenes, types as T
from interpolate_ref import interpolate_ref, ray_matrix32

SIZES = [(1, 1), (31, 7), (33, 9), (64, 8), (65, 17), (129, 3)]
TS = [0.0, 0.25, 0.5, 1.0]
RADII = [0, 1, 4, 8]
MAIN = (96, 54)
LARGE = (320, 180)

EYE = np.array([0.0, 0.0, 15.0])
# the poses: (offset along right, up, forward) of the eye
POSES = {"a": (-0.6, 0.0, 0.0), "mid": (0.0, 0.5, 0.0), "b": (0.6, 0.0, 0.0)}
WALL, EDGE_U, TILT = 6.0, 0.9, 0.8   # depth of the left wall, the edge, the right wall's slope towards the viewer
TOP = 2.2                            # the walls end here: misses above
DISC = (-0.5, 0.2, 4.0, 0.9)         # u, v, depth, radius
TAG = (-0.9, -0.6, 1.42, 1.55)       # u0, u1, v0, v1 on the left wall: hidden behind the disc's rim from A and from B
EMITTER = (1.6, 2.6, -1.5, -0.5)     # on the right wall
MIRROR = (-3.2, -2.2, -1.8, -0.6)    # on the left wall
COLOURS = {0: (0.7, 0.3, 0.2), 1: (0.2, 0.5, 0.7), 2: (0.9, 0.9, 0.2), 3: (5.0, 5.0, 5.0), 4: (0.9, 0.9, 0.9), 5: (0.1, 0.8, 0.3), -1: (0.3, 0.4, 0.6)}


def camera(w, h, pose):
    """The FfCamera of pose "a", "mid" or "b" (or an (du, dv, dd) offset of the eye) for a w x h image."""
    du, dv, dd = POSES[pose] if isinstance(pose, str) else pose
    base = scenes.default_camera(w, h)
    R, U, F = (np.array(v.tuple(), np.float64) for v in (base.m_right, base.m_up, base.m_forward))
    return scenes.posed_camera(w, h, tuple(EYE + du * R + dv * U + dd * F), base.m_yaw, base.m_pitch)


def view(w, h, pose, disc_shift=(0.0, 0.0)):
    """(camera, position [h,w,3] float32, ids [h,w,3] int32) of the scene from a pose; disc_shift moves the disc in (u, v)."""
    cam = camera(w, h, pose)
    base = scenes.default_camera(w, h)
    R, U, F = (np.array(v.tuple(), np.float64) for v in (base.m_right, base.m_up, base.m_forward))
    M = ray_matrix32(cam).astype(np.float64).reshape(4, 4).T
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    far = float(cam.m_farClip)
    v4 = np.stack([(xs / w * 2 - 1) * far, (1 - ys / h * 2) * far, np.full_like(xs, far), np.full_like(xs, far)], -1)
    eye = np.array(cam.m_position.tuple(), np.float64)
    d = (v4 @ M.T)[..., :3] - eye
    # into the scene's frame (u along right, v along up, z along forward, from EYE)
    o = np.array([(eye - EYE) @ R, (eye - EYE) @ U, (eye - EYE) @ F])
    d = np.stack([d @ R, d @ U, d @ F], -1)
    best = np.full((h, w), np.inf)
    ids = np.full((h, w, 3), -1, np.int32)
    hit_at = np.zeros((h, w, 3))

    def take(s, ok, geom, kind, patch=False):
        nonlocal best, hit_at
        p = o + s[..., None] * d
        ok = ok & (s > 0) & ((s <= best) if patch else (s < best))  # (a patch lies in its wall)
        best = np.where(ok, s, best)
        hit_at = np.where(ok[..., None], p, hit_at)
        ids[ok] = (geom, -1, kind)
        return p

    def box(p, b):
        return (p[..., 0] >= b[0]) & (p[..., 0] < b[1]) & (p[..., 1] >= b[2]) & (p[..., 1] < b[3])

    with np.errstate(divide="ignore", invalid="ignore"):
        s = (WALL - o[2]) / d[..., 2]                                  # the left wall z = WALL, u < EDGE_U
        p = o + s[..., None] * d
        on = (p[..., 0] < EDGE_U) & (p[..., 1] < TOP)
        take(s, on, 0, T.BXDF_DIFFUSE)
        take(s, on & box(p, MIRROR), 4, T.BXDF_MIRROR, True)
        take(s, on & box(p, TAG), 5, T.BXDF_DIFFUSE, True)
        n = np.array([TILT, 0.0, 1.0])                                 # the right wall z = WALL - TILT (u - EDGE_U), u >= EDGE_U
        s = (WALL + TILT * EDGE_U - o @ n) / (d @ n)
        p = o + s[..., None] * d
        on = (p[..., 0] >= EDGE_U) & (p[..., 1] < TOP)
        take(s, on, 1, T.BXDF_DIFFUSE)
        take(s, on & box(p, EMITTER), 3, T.BXDF_EMITTER, True)
        s = (DISC[2] - o[2]) / d[..., 2]                               # the disc
        p = o + s[..., None] * d
        du, dv = p[..., 0] - (DISC[0] + disc_shift[0]), p[..., 1] - (DISC[1] + disc_shift[1])
        take(s, du * du + dv * dv < DISC[3] ** 2, 2, T.BXDF_DIFFUSE)
    world = EYE + hit_at[..., :1] * R + hit_at[..., 1:2] * U + hit_at[..., 2:] * F
    pos = np.where((ids[..., :1] >= 0), world, 0.0).astype(np.float32)
    return cam, pos, ids


def radiance(pos, ids, seed, shade=0.15):
    """A finite radiance over a view: the geometry's colour under a light that varies smoothly with the WORLD point (so the two
    sources agree about a surface point up to `shade` times seeded noise); the sky varies with the pixel."""
    rng = np.random.default_rng(seed)
    h, w = ids.shape[:2]
    col = np.zeros((h, w, 3))
    for g, c in COLOURS.items():
        col[ids[..., 0] == g] = c
    light = 0.7 + 0.3 * np.sin(pos[..., :1].astype(np.float64) * 2.0 + pos[..., 1:2] * 1.3)
    return (col * light * (1.0 + shade * rng.uniform(-1, 1, (h, w, 3)))).astype(np.float32)


def disc_maps(shift_a, shift_b, n=6):
    """geom_maps [n,2,3,4] for a disc (geometry 2) that stands at DISC at the mid pose and is moved by shift_S = (du, dv) at S."""
    base = scenes.default_camera(8, 8)
    R, U = (np.array(v.tuple(), np.float64) for v in (base.m_right, base.m_up))
    maps = np.tile(np.eye(3, 4, dtype=np.float32), (n, 2, 1, 1))
    for S, sh in enumerate((shift_a, shift_b)):
        maps[2, S, :, 3] = (sh[0] * R + sh[1] * U).astype(np.float32)
    return maps


_CACHE = {}


def case(size, moving=False):
    """dict(mid=(camera, position, ids), a=(camera, radiance, position, ids), b=..., maps=None or [6,2,3,4]) at `size`; cached and
    read-only.  moving: the disc stands 0.1 to the left at A and 0.1 to the right at B, carried by a geometry map."""
    key = (size, moving)
    if key not in _CACHE:
        w, h = size
        sa, sb = ((-0.1, 0.0), (0.1, 0.02)) if moving else ((0.0, 0.0), (0.0, 0.0))
        cm, pm, im = view(w, h, "mid")
        ca, pa, ia = view(w, h, "a", sa)
        cb, pb, ib = view(w, h, "b", sb)
        c = {"mid": (cm, pm, im), "a": (ca, radiance(pa, ia, 11), pa, ia), "b": (cb, radiance(pb, ib, 12), pb, ib),
             "maps": disc_maps(sa, sb) if moving else None}
        for arrs in (c["mid"][1:], c["a"][1:], c["b"][1:]):
            for x in arrs:
                x.setflags(write=False)
        _CACHE[key] = c
    return _CACHE[key]


def with_radiance(c, rad_a=None, rad_b=None):
    """The case with other source radiances."""
    a, b = c["a"], c["b"]
    return dict(c, a=(a[0], a[1] if rad_a is None else rad_a, a[2], a[3]), b=(b[0], b[1] if rad_b is None else rad_b, b[2], b[3]))


def planted_nonfinite(c, seed=5, count=40):
    """The case with NaN, +Inf and -Inf planted in single channels of both sources (other places in A than in B)."""
    rng = np.random.default_rng(seed)
    out = []
    for rad in (c["a"][1], c["b"][1]):
        r = rad.copy()
        h, w = r.shape[:2]
        for i in range(count):
            r[rng.integers(h), rng.integers(w), rng.integers(3)] = (np.nan, np.inf, -np.inf)[i % 3]
        out.append(r)
    return with_radiance(c, *out)


def seam_holes(size=(70, 20)):
    """Three bitwise-equal cameras and G-buffers (every pixel is its own tap), with both sources non-finite - so the pixel is a hole
    - on both sides of the fill kernel's tile seams x = 31|32 and y = 7|8, at a tile's corner, at the image's corner and in a block
    wider than the fill radius; the rest of A and B differ.  -> (case, hole mask [h,w])."""
    w, h = size
    cm, pm, im = view(w, h, "mid")
    ra, rb = radiance(pm, im, 21), radiance(pm, im, 22)
    hole = np.zeros((h, w), bool)
    for y, x in ((3, 31), (3, 32), (7, 10), (8, 10), (7, 31), (8, 32), (7, 32), (8, 31), (0, 0), (h - 1, w - 1), (15, 63), (16, 64)):
        hole[y, x] = True
    hole[10:14, 40:52] = True
    ra[hole] = np.nan
    rb[hole, 1] = np.inf
    return {"mid": (cm, pm, im), "a": (cm, ra, pm, im), "b": (cm, rb, pm, im), "maps": None}, hole


def ref(c, **params):
    """interpolate_ref of a case."""
    return interpolate_ref(c["mid"], c["a"], c["b"], geom_maps=c["maps"], **params)


def main_counts():
    """The restatement's five counts on the main case (MAIN, the defaults): each must be nonzero, or the parity tests exercise
    nothing."""
    return ref(case(MAIN))[2]
