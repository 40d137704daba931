"""Planted inputs for the tile-max skeleton ff_motion_blur and ff_depth_of_field share (csrc/ff_tile_filter.h): what the host test
(test_tile_filter_host.py) and the GPU test (test_gpu_tile_filter.py) both build.  Deterministic: a seed fixed by (w, h, k).

A tile's maximum T is seen only through the gather, and only where it is the largest of a 3 x 3 block of tiles (N).  So every
input here has DOMINANT tiles, whose plant is larger than every other tile's, and a plan says which tiles those are and at which
in-tile row-major index each tile's plant sits.  A plan is a dict:

  phase      (px, py): the tiles with tx % 3 == px and ty % 3 == py are dominant (every 3 x 3 block holds exactly one); None: none
  rot        which of its admissible positions (positions_of) a tile's plant takes: a dominant tile the rot-th, tile t the
             (rot + t)-th, both modulo the tile's count
  tie        motion only: every dominant tile carries a TIE PLANT, two pixels at its rot-th and (rot + 1)-th positions with
             bit-identical |v|^2, (a, b) at the earlier index and (b, a) at the later one.  The later one must lose
  tile_ties  motion only: pairs ((tx, ty), (tx2, ty2)) of tiles, the first earlier in row-major order.  Both get one dominant
             magnitude, (a, b) in the first and (b, a) in the second: a TILE TIE.  The first of a 3 x 3 block must win
  clamp      depth of field only: the dominant tiles' plants lie nearer than the clamp: their l is exactly k
  misses     depth of field only: the tile (row-major index) that holds only misses

All motion is built for SHUTTER = 1: the half-spread is v = 0.5 m, and m = 2 v is exact."""
import functools

import numpy as np

from dof_cases import camera  # noqa: F401  (the tests take the camera from here)

F = np.float32
SHUTTER = 1.0
FOCUS = 2.0
# every tile width the skeleton treats differently: one lane per tile, the lane groups of 4, 16, 32 and 64 (with and without idle
# lanes), one workgroup per tile with idle waves (9, 12, 15), exactly one trip (16), a partial second trip (17, 23), whole trips
# (32, 64) and a partial last trip (33, 63)
KS = [1, 2, 4, 5, 6, 8, 9, 12, 15, 16, 17, 23, 32, 33, 63, 64]


def size_for(k):
    """The smallest image with full tiles, a partial tile on each axis, a corner tile and 3 x 3 tiles or more (from k = 4 on exactly
    3 tiles a side: two full ones and a partial one, which is all k >= 32 can afford and all N needs for an interior tile)."""
    w, h = 2 * k + k // 2 + 1, 2 * k + 3
    return w + (k > 1 and w % k == 0), h + (k > 1 and h % k == 0)  # (k = 2: 6 x 7 has no partial column, 7 x 7 has)


def grid_of(w, h, k):
    return (w + k - 1) // k, (h + k - 1) // k


def tile_box(w, h, k, tx, ty):
    """(x0, y0, tw, th) of tile (tx, ty)."""
    x0, y0 = tx * k, ty * k
    return x0, y0, min(k, w - x0), min(k, h - y0)


def positions_of(tw, th, k):
    """The in-tile row-major indices a plant is put at, as far as a tw x th tile of a k-grid has them: the first two pixels, the
    last one (tw th - 1: it depends on the clipped size), the first of the second row (tw: it depends on the clipped width), both
    sides of a wave's edge (63, 64) and of the strided loop's second trip (255, 256), and for k <= 8 the last lane of the lane
    group that holds a pixel of a full tile (k k - 1)."""
    cand = [0, 1, tw * th - 1, tw, 63, 64, 255, 256] + ([k * k - 1] if k <= 8 else [])
    return sorted({i for i in cand if 0 <= i < tw * th})


def pixel_of(w, h, k, tx, ty, i):
    """(y, x) in the image of pixel i (row-major) of tile (tx, ty)."""
    x0, y0, tw, th = tile_box(w, h, k, tx, ty)
    assert 0 <= i < tw * th
    return y0 + i // tw, x0 + i % tw


def is_dominant(plan, tx, ty):
    return plan.get("phase") is not None and (tx % 3, ty % 3) == tuple(plan["phase"])


def shape_tiles(w, h, k):
    """One tile of every shape: full at the corner, interior, clipped at the right, at the bottom, and at both."""
    nx, ny = grid_of(w, h, k)
    tiles = [(0, 0), (min(1, nx - 1), min(1, ny - 1)), (nx - 1, 0), (0, ny - 1), (nx - 1, ny - 1)]
    return sorted(set(tiles), key=lambda t: (t[1], t[0]))


SHAPES = ["first", "interior", "right", "bottom", "corner"]  # shape_tiles' order where the image has 3 x 3 tiles or more


def plan_groups(w, h, k, ties=True):
    """Every plan the planted tests run at (w, h, k), one group per shape of tile: that tile dominant with its plant at each of its
    positions in turn; with `ties`, also a tie plant at each pair of neighbouring positions, and one tile tie per group: beside,
    below (each at the first tile and at the clipped corner) and diagonally."""
    nx, ny = grid_of(w, h, k)
    groups = []
    for tx, ty in shape_tiles(w, h, k):
        _, _, tw, th = tile_box(w, h, k, tx, ty)
        n = len(positions_of(tw, th, k))
        groups.append([dict(phase=(tx % 3, ty % 3), rot=r) for r in range(n)])
        if ties:
            groups[-1] += [dict(phase=(tx % 3, ty % 3), rot=r, tie=True) for r in range(n - 1)]
    if ties:
        pairs = []
        if nx > 1:
            pairs += [((0, 0), (1, 0)), ((nx - 2, ny - 1), (nx - 1, ny - 1))]
        if ny > 1:
            pairs += [((0, 0), (0, 1)), ((nx - 1, ny - 2), (nx - 1, ny - 1))]
        if nx > 1 and ny > 1:
            pairs += [((1, 0), (0, 1))]  # (row-major: the upper right tile comes before the lower left one)
        for r, pair in enumerate(pairs):
            groups[r % len(groups)].append(dict(phase=None, rot=r, tile_ties=[pair]))
    return groups


def plans_for(w, h, k, ties=True):
    return [plan for group in plan_groups(w, h, k, ties) for plan in group]


def _unit(t):
    """A number in [0, 1) that differs from tile to tile (the golden-ratio sequence)."""
    return ((t + 1) * 0.6180339887498949) % 1.0


@functools.lru_cache(maxsize=None)
def _radiance(w, h, k):
    rng = np.random.default_rng(15485863 * w + 32452843 * h + k)
    rad = np.exp2(rng.uniform(-8.0, 4.0, (h, w, 3))).astype(np.float32)
    rad.setflags(write=False)
    return rad


# ---- motion blur ----------------------------------------------------------------------------------------------------------------

def motion_bands(k):
    """(baseline, plant, dominant) half-spreads in pixels, each a (low, high) band.  The baseline is clearly below the plants and,
    from k = 2 on, above 0.5 px and a third of k: long enough that the taps along N's direction weigh in at every pixel.  At k = 1
    a tap (one pixel away) counts only between two pixels of l > 1 / 1.05 = 0.952 (the cylinder term), so everything lies above."""
    if k == 1:
        return (0.955, 0.962), (0.968, 0.978), (0.986, 0.998)
    return (0.30 * k, 0.45 * k), (0.60 * k, 0.85 * k), (0.90 * k, 0.985 * k)


def _vector(k, magnitude, angle_unit, plant=True):
    """A half-spread of the given length.  At k = 1 within 0.3 rad of an axis (a diagonal tap is sqrt 2 away and never counts);
    elsewhere anywhere, and never within 0.1 rad of an axis or a diagonal, so that (a, b) and (b, a) are different directions.
    A plant's components have one sign: the taps of the image's first and last pixel, which are plant positions, then stay inside
    the image on one side, and taking the plant away is seen there too."""
    span = 0.2 if k == 1 else np.pi / 4 - 0.2
    octant, frac = divmod(angle_unit * 8.0, 1.0)
    if plant:
        octant = (0, 1, 4, 5)[int(octant) % 4]
    quadrant, upper = divmod(int(octant), 2)
    angle = quadrant * (np.pi / 2) + (np.pi / 2 - 0.1 - span * frac if upper else 0.1 + span * frac)
    return F(magnitude * np.cos(angle)), F(magnitude * np.sin(angle))


def motion_plants(w, h, k, plan):
    """The plants of a plan: a list of dicts {tile, pixel (y, x), index, v (half-spread), kind}, kind one of 'plant', 'dominant',
    'tie_first', 'tie_second', 'tile_tie_first', 'tile_tie_second'."""
    nx, ny = grid_of(w, h, k)
    _, band, top = motion_bands(k)
    rot = plan.get("rot", 0)
    tied = {}
    for n, (first, second) in enumerate(plan.get("tile_ties", ())):
        assert first[1] * nx + first[0] < second[1] * nx + second[0]
        a, b = _vector(k, top[0] + (top[1] - top[0]) * _unit(7 * n + 3), _unit(5 * n + 1))
        tied[tuple(first)] = ((a, b), "tile_tie_first")
        tied[tuple(second)] = ((b, a), "tile_tie_second")
    out = []
    for ty in range(ny):
        for tx in range(nx):
            t = ty * nx + tx
            _, _, tw, th = tile_box(w, h, k, tx, ty)
            pos = positions_of(tw, th, k)
            rec = lambda i, v, kind: dict(tile=(tx, ty), index=i, pixel=pixel_of(w, h, k, tx, ty, i), v=v, kind=kind)  # noqa: E731
            if (tx, ty) in tied:
                v, kind = tied[(tx, ty)]
                out.append(rec(pos[(rot + t) % len(pos)], v, kind))
            elif is_dominant(plan, tx, ty):
                a, b = _vector(k, top[0] + (top[1] - top[0]) * _unit(t), _unit(3 * t + 2))
                if plan.get("tie") and len(pos) > 1:
                    r = rot % (len(pos) - 1)
                    out.append(rec(pos[r], (a, b), "tie_first"))
                    out.append(rec(pos[r + 1], (b, a), "tie_second"))
                else:
                    out.append(rec(pos[rot % len(pos)], (a, b), "dominant"))
            else:
                out.append(rec(pos[(rot + t) % len(pos)], _vector(k, band[0] + (band[1] - band[0]) * _unit(t), _unit(3 * t + 2)), "plant"))
    return out


@functools.lru_cache(maxsize=None)
def motion_baseline(w, h, k):
    """(motion, depth) without plants: every pixel moves, in its own direction, by a half-spread inside the baseline band."""
    rng = np.random.default_rng(49979687 * w + 67867967 * h + k)
    base, _, _ = motion_bands(k)
    magnitude = rng.uniform(base[0], base[1], (h, w))
    angle = rng.random((h, w))
    motion = np.empty((h, w, 2), np.float32)
    for y in range(h):
        for x in range(w):
            a, b = _vector(k, magnitude[y, x], angle[y, x], plant=False)
            motion[y, x] = (a * F(2), b * F(2))
    depth = rng.uniform(0.5, 6.0, (h, w)).astype(np.float32)
    depth[rng.random((h, w)) < 0.1] = 0.0
    for a in (motion, depth):
        a.setflags(write=False)
    return motion, depth


def with_motion_plants(motion, plants):
    out = np.array(motion)
    for p in plants:
        out[p["pixel"]] = (p["v"][0] * F(2), p["v"][1] * F(2))
    return out


PLANT_DEPTH = 0.25  # nearer than every baseline pixel


def planted_motion(w, h, k, plan):
    """(rad, motion, depth) for ff_motion_blur at shutter SHUTTER and max_radius k.  A plant is foreground: at a miss (which the
    baseline has) nothing of its spread would show under a small k."""
    motion, depth = motion_baseline(w, h, k)
    plants = motion_plants(w, h, k, plan)
    depth = np.array(depth)
    for p in plants:
        depth[p["pixel"]] = PLANT_DEPTH
    return _radiance(w, h, k), with_motion_plants(motion, plants), depth


# ---- depth of field -------------------------------------------------------------------------------------------------------------

def dof_bands(k):
    """(baseline, plant, dominant) circle-of-confusion radii in pixels.  The baseline is near focus, 0.6 .. 2 px where k allows."""
    base = (0.6, max(0.66, min(2.0, 0.45 * k)))
    return base, (max(0.55 * k, base[1] + 0.05), 0.80 * k), (0.88 * k, 0.97 * k)


def dof_coc_scale(k):
    """So that a miss (at infinity: l = coc_scale / FOCUS) lies in the middle of the baseline band."""
    base, _, _ = dof_bands(k)
    return float(F(FOCUS * 0.5 * (base[0] + base[1])))


def _axial(k, l):
    """The axial depth in front of the focus plane at which the radius is l: l = coc_scale (1 / z - 1 / FOCUS)."""
    return F(1.0 / (1.0 / FOCUS + l / dof_coc_scale(k)))


def dof_plants(w, h, k, plan):
    """The plants of a plan: a list of dicts {tile, pixel (y, x), index, z (axial depth), kind}, kind 'plant', 'dominant' or 'clamped'."""
    nx, ny = grid_of(w, h, k)
    _, band, top = dof_bands(k)
    rot = plan.get("rot", 0)
    out = []
    for ty in range(ny):
        for tx in range(nx):
            t = ty * nx + tx
            if t == plan.get("misses"):
                continue
            _, _, tw, th = tile_box(w, h, k, tx, ty)
            pos = positions_of(tw, th, k)
            if is_dominant(plan, tx, ty):
                i = pos[rot % len(pos)]
                l, kind = (1.5 * k, "clamped") if plan.get("clamp") else (top[0] + (top[1] - top[0]) * _unit(t), "dominant")
            else:
                i = pos[(rot + t) % len(pos)]
                l, kind = band[0] + (band[1] - band[0]) * _unit(t), "plant"
            out.append(dict(tile=(tx, ty), index=i, pixel=pixel_of(w, h, k, tx, ty, i), z=_axial(k, l), kind=kind))
    return out


@functools.lru_cache(maxsize=None)
def dof_baseline(w, h, k):
    """(position, depth) without plants, for camera(w, h) (at the origin, looking down -z): every pixel a hit on the axis, in front
    of or behind the focus plane, with a radius inside the baseline band."""
    rng = np.random.default_rng(86028121 * w + 98764321 * h + k)
    base, _, _ = dof_bands(k)
    l = rng.uniform(base[0], base[1], (h, w))
    near = rng.random((h, w)) < 0.5
    scale = dof_coc_scale(k)
    inverse = np.where(near, 1.0 / FOCUS + l / scale, np.maximum(1.0 / FOCUS - l / scale, 1.0e-3))  # (behind: at most a miss's radius)
    pos = np.zeros((h, w, 3), np.float32)
    pos[..., 2] = -(1.0 / inverse)
    depth = np.abs(pos[..., 2]).astype(np.float32)
    for a in (pos, depth):
        a.setflags(write=False)
    return pos, depth


def with_dof_plants(w, h, k, pos, depth, plants, plan):
    pos, depth = np.array(pos), np.array(depth)
    if plan.get("misses") is not None:
        nx, _ = grid_of(w, h, k)
        x0, y0, tw, th = tile_box(w, h, k, plan["misses"] % nx, plan["misses"] // nx)
        pos[y0:y0 + th, x0:x0 + tw] = 0.0
        depth[y0:y0 + th, x0:x0 + tw] = 0.0
    for p in plants:
        pos[p["pixel"]] = (0.0, 0.0, -p["z"])
        depth[p["pixel"]] = p["z"]
    return pos, depth


def planted_positions(w, h, k, plan, cam=None):
    """(rad, position, depth) for ff_depth_of_field under camera(w, h) with focus FOCUS, coc_scale dof_coc_scale(k), max_radius k.
    `cam` is only checked: the planes are built for a camera at the origin that looks down -z."""
    if cam is not None:
        assert (cam.m_position.x, cam.m_position.y, cam.m_position.z) == (0.0, 0.0, 0.0) and cam.m_forward.z == -1.0
    pos, depth = dof_baseline(w, h, k)
    pos, depth = with_dof_plants(w, h, k, pos, depth, dof_plants(w, h, k, plan), plan)
    return _radiance(w, h, k), pos, depth


def dof_plan_groups(w, h, k):
    """plan_groups without ties, the tile after the first dominant one holding only misses; and for every shape of tile one plan
    with the dominant plant clamped to exactly k."""
    nx, ny = grid_of(w, h, k)
    groups = []
    for group in plan_groups(w, h, k, ties=False):
        groups.append([])
        for plan in group:
            first = next(t for t in range(nx * ny) if is_dominant(plan, t % nx, t // nx))
            plan["misses"] = (first + 1) % (nx * ny)
            groups[-1].append(plan)
            if plan["rot"] == 0:
                groups[-1].append(dict(plan, clamp=True))
    return groups


def dof_plans_for(w, h, k):
    return [plan for group in dof_plan_groups(w, h, k) for plan in group]


# ---- many tiles per workgroup ---------------------------------------------------------------------------------------------------

STRADDLE_SIZE = (160, 90)
STRADDLE_KS = [1, 2, 4]  # a lane, 4 lanes and 16 lanes per tile: 256, 64 and 16 tiles per workgroup of 256 threads
NARROW = [(12, 7, 30), (12, 30, 7), (33, 20, 70), (33, 70, 20)]  # (k, w, h): w < k < h and h < k < w, a column and a row of clipped tiles


def straddle_plan(k):
    """Tile ties across the seams between workgroups of the lane-group kernel (tile index a multiple of 256 / lanes per tile): two
    tiles side by side on either side of a seam in the middle of a row of tiles, and further down one above the other, in different
    workgroups.  No dominant tiles: every tile's plant has its own magnitude, and N chooses among nine of them."""
    w, h = STRADDLE_SIZE
    nx, ny = grid_of(w, h, k)
    per = 256 // {1: 1, 2: 4, 4: 16}[k]
    seams = [b for b in range(per, nx * ny, per) if b % nx]
    beside = seams[0]
    below = next(b for b in seams if b // nx >= beside // nx + 3)
    at = lambda t: (t % nx, t // nx)  # noqa: E731
    return dict(phase=None, rot=1, tile_ties=[(at(beside - 1), at(beside)), (at(below - nx), at(below))])


# ---- the references, computed once ------------------------------------------------------------------------------------------------

_REFERENCES = {}


def motion_reference(rad, motion, depth, p, key):
    """motion_blur_ref's answer, kept under `key` (a case's name and plan) for the tests that share the case."""
    import motion_blur_ref
    from motion_blur_cases import params_of
    if ("motion", key) not in _REFERENCES:
        _REFERENCES[("motion", key)] = motion_blur_ref.motion_blur(rad, motion, depth, **params_of(p))
    return _REFERENCES[("motion", key)]


def dof_reference(rad, pos, depth, cam, p, key):
    from dof_cases import reference
    if ("dof", key) not in _REFERENCES:
        _REFERENCES[("dof", key)] = reference(rad, pos, depth, cam, p)
    return _REFERENCES[("dof", key)]


def block_mask(w, h, k, tx, ty):
    """The pixels of the 3 x 3 tiles around tile (tx, ty)."""
    mask = np.zeros((h, w), bool)
    mask[max(ty - 1, 0) * k:(ty + 2) * k, max(tx - 1, 0) * k:(tx + 2) * k] = True
    return mask


# ---- degenerate guides ----------------------------------------------------------------------------------------------------------

DENORMAL = float(np.float32(1e-45))

# motion that is no motion by ff_api.h step 1.  NaN and Inf: v is not finite.  1e30: v.x v.x is Inf, so l is Inf, s = k / l = 0 and
# the kept v is 0.  (3e19, 3e19): each square is finite (2.25e38 < FLT_MAX) and their sum is Inf, the same way.  A denormal: v.x v.x
# underflows to 0, l = 0, and its key ties with a pixel at rest.
BAD_MOTION = [(np.nan, 3.0), (np.inf, 0.0), (5.0, -np.inf), (1e30, 0.0), (-1e30, 1e30), (3e19, 3e19), (DENORMAL, -DENORMAL)]
# depth that is a miss by ff_api.h step 1 (not finite, or not > 0)
BAD_DEPTH = [np.nan, np.inf, -np.inf, -2.0, 0.0]
# positions that are a miss: not finite (e is NaN or Inf, so z is), behind the camera, and at axial depth 1e-6 exactly (not > 1e-6f)
BAD_POSITION = [(np.nan, 0.0, -1.0), (0.0, np.inf, -1.0), (0.0, 0.0, -np.inf), (0.0, 0.0, np.inf), (0.0, 0.0, 1.0), (0.0, 0.0, 0.0),
                (0.0, 0.0, -float(np.float32(1e-6)))]
DEGENERATE_KS = [4, 12, 33]  # a lane group per tile, one partly idle workgroup per tile, more than one trip


def degenerate_plan(w, h, k):
    return dict(phase=(1, 1), rot=2)


def planted_dof_params(k, **overrides):
    from gpupathtracer_amd import lib
    return lib.dof_params(**dict(dict(focus_distance=FOCUS, coc_scale=dof_coc_scale(k), max_radius=k, grid=3), **overrides))


def degenerate_motion_cases(k):
    """(name, inputs, the inputs whose output must be the same bit for bit or None, inputs whose output must differ) at size_for(k),
    the bad values in the pixels that win their tiles, the dominant tile's first."""
    w, h = size_for(k)
    plan = degenerate_plan(w, h, k)
    rad, motion, depth = planted_motion(w, h, k, plan)
    plants = motion_plants(w, h, k, plan)
    bad, as_zero = spoil(motion, plants, BAD_MOTION, 0.0)
    bad_depth, as_miss = spoil(depth, plants, BAD_DEPTH, 0.0)
    tiny, one_miss = spoil(depth, plants, [DENORMAL], 0.0)
    return [("motion", (rad, bad, depth), (rad, as_zero, depth), (rad, motion, depth)),
            ("motion and depth", (rad, bad, bad_depth), (rad, as_zero, as_miss), (rad, motion, depth)),
            ("depth 1e-45", (rad, motion, tiny), None, (rad, motion, one_miss))]


def degenerate_dof_cases(k):
    """(name, inputs, the inputs whose output must be the same bit for bit or None, inputs whose output under the planted parameters
    must differ, parameter overrides) at size_for(k) under camera(*size_for(k))."""
    w, h = size_for(k)
    plan = dict(degenerate_plan(w, h, k), misses=0)
    rad, pos, depth = planted_positions(w, h, k, plan)
    plants = dof_plants(w, h, k, plan)
    bad_pos, miss_pos = spoil(pos, plants, BAD_POSITION, 0.0)
    _, miss_depth = spoil(depth, plants, [1.0] * len(BAD_POSITION), 0.0)
    bad_depth, as_miss = spoil(depth, plants, BAD_DEPTH, 0.0)
    tiny, one_miss = spoil(depth, plants, [DENORMAL], 0.0)
    far, _ = spoil(pos, plants, [(0.0, 0.0, -1e30)], 0.0)
    planted = (rad, pos, depth)
    return [("positions", (rad, bad_pos, depth), (rad, miss_pos, miss_depth), planted, {}),
            ("depth", (rad, pos, bad_depth), (rad, pos, as_miss), planted, {}),
            ("depth 1e-45", (rad, pos, tiny), planted, (rad, pos, one_miss), {}),
            ("position 1e30 ahead", (rad, far, depth), None, planted, {}),
            ("coc_scale 1e30", (rad, bad_pos, bad_depth), None, planted, dict(coc_scale=1e30))]


def spoil(plane, plants, values, as_value):
    """Two copies of `plane`: the plants' pixels, the dominant tile's first, set to `values` in turn in one and to `as_value` in the
    other."""
    order = sorted(plants, key=lambda p: p["kind"] == "plant")
    assert len(values) <= len(order)
    bad, clean = np.array(plane), np.array(plane)
    for p, value in zip(order, values):
        bad[p["pixel"]] = value
        clean[p["pixel"]] = as_value
    return bad, clean
