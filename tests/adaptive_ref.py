"""numpy float32 restatement of ff_render_adaptive (include/firefly/ff_api.h): the tile error with its fixed order of adds, the
rectangle plan, and the whole driver over a callback render(seed, x0, y0, w, h) -> float32 [h, w, 3].  Nothing here calls the
library: the tests hold the host twin and the device against it bit for bit."""
import numpy as np

F = np.float32
LANES = 256


def bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


def tile_grid(width, height, tile):
    """(tiles_y, tiles_x)."""
    return (height + tile - 1) // tile, (width + tile - 1) // tile


def tile_box(width, height, tile, tx, ty):
    """(x0, y0, x1, y1) of tile (tx, ty) in pixels: narrower and shorter at the right and bottom edges."""
    return tx * tile, ty * tile, min(width, (tx + 1) * tile), min(height, (ty + 1) * tile)


def pixel_errors(sum_all, sum_even, n):
    """e_p of every pixel after n passes (n even), float32 [H, W]."""
    s, se = np.asarray(sum_all, dtype=F), np.asarray(sum_even, dtype=F)
    inv_n, inv_h = F(1.0) / F(n), F(1.0) / F(n // 2)
    with np.errstate(all="ignore"):
        i, a = s * inv_n, se * inv_h
        d = (i[..., 0] + i[..., 1]) + i[..., 2]
        num = (np.abs(i[..., 0] - a[..., 0]) + np.abs(i[..., 1] - a[..., 1])) + np.abs(i[..., 2] - a[..., 2])
        e = np.where(d > 0, num / np.sqrt(d), F(0.0)).astype(F)  # (!(d > 0): also a NaN d gives 0)
    assert i.dtype == F and e.dtype == F
    return e


def ordered_sum(e):
    """S of a tile's errors e (1-D, the tile's row-major order): lane j of 256 adds e_j, e_(j+256), ... from 0.0f, then the halving
    tree v[j] += v[j + off], off = 128 .. 1."""
    e = np.asarray(e, dtype=F).reshape(-1)
    rows = (e.size + LANES - 1) // LANES
    padded = np.zeros(rows * LANES, dtype=F)  # (a trailing + 0.0f changes no lane: every lane starts from +0.0f)
    padded[:e.size] = e
    v = np.zeros(LANES, dtype=F)
    with np.errstate(all="ignore"):
        for row in padded.reshape(rows, LANES):
            v = v + row
        off = LANES // 2
        while off >= 1:
            v[:off] = v[:off] + v[off:2 * off]
            off //= 2
    return v[0]


def scale(S, tile_pixels, image_pixels):
    """E_t = S * sqrt((float)N_t / (float)(W * H)) / (float)N_t, left to right."""
    with np.errstate(all="ignore"):
        n_t = F(tile_pixels)
        return F(F(S * np.sqrt(n_t / F(image_pixels))) / n_t)


def tile_errors(sum_all, sum_even, tile, n, order=None):
    """E_t of every tile, float32 [tiles_y, tiles_x].  order: a function that permutes a tile's 1-D error vector before the sum (the
    order test); None: the specified order."""
    h, w = np.asarray(sum_all).shape[:2]
    e = pixel_errors(sum_all, sum_even, n)
    tiles_y, tiles_x = tile_grid(w, h, tile)
    out = np.zeros((tiles_y, tiles_x), dtype=F)
    for ty in range(tiles_y):
        for tx in range(tiles_x):
            x0, y0, x1, y1 = tile_box(w, h, tile, tx, ty)
            v = e[y0:y1, x0:x1].reshape(-1)
            if order is not None:
                v = order(v)
            out[ty, tx] = scale(ordered_sum(v), v.size, w * h)
    return out


def plan(active):
    """The rectangle list of a [tiles_y, tiles_x] array of flags, int32 [n, 4] of {tx0, ty0, tx1, ty1} (tiles, half open): per row
    the maximal runs of active tiles; a run continues the rectangle that reached the row above with the identical span."""
    active = np.asarray(active) != 0
    rects, open_ = [], {}
    for ty, row in enumerate(active):
        runs, tx = [], 0
        while tx < row.size:
            if not row[tx]:
                tx += 1
                continue
            end = tx
            while end < row.size and row[end]:
                end += 1
            runs.append((tx, end))
            tx = end
        reached = {}
        for span in runs:
            if span in open_:
                rects[open_[span]][3] = ty + 1
                reached[span] = open_[span]
            else:
                rects.append([span[0], ty, span[1], ty + 1])
                reached[span] = len(rects) - 1
        open_ = reached
    return np.array(rects, dtype=np.int32).reshape(-1, 4)


def to_u8(v):
    """The project's 8-bit rule: trunc(clamp(v * 255)), NaN -> 0."""
    with np.errstate(all="ignore"):
        s = np.asarray(v, dtype=F) * F(255.0)
        return np.where(s > 0, np.where(s >= 255, 255, np.trunc(np.where(np.isfinite(s), s, 0))), 0).astype(np.uint8)


def neighbours(tiles_y, tiles_x, ty, tx):
    return [(qy, qx) for qy in range(ty - 1, ty + 2) for qx in range(tx - 1, tx + 2)
            if (qy, qx) != (ty, tx) and 0 <= qy < tiles_y and 0 <= qx < tiles_x]


def drive(render, width, height, seed, tile, min_passes, max_passes, threshold, guard=False):
    """The driver.  -> dict: sum, sum_even [H,W,3]; tile_passes [ty,tx] uint16; tile_error [ty,tx]; radiance, rgb8, passes [H,W];
    passes_run, rectangles, pixels_rendered (the sum over the rectangles: samples / spp); checks: one dict per check with n, error
    (the tiles' errors after it), active_before and stopped (boolean tile arrays)."""
    tiles_y, tiles_x = tile_grid(width, height, tile)
    threshold = F(threshold)
    total = np.zeros((height, width, 3), dtype=F)
    even = np.zeros((height, width, 3), dtype=F)
    active = np.ones((tiles_y, tiles_x), dtype=bool)
    tile_passes = np.zeros((tiles_y, tiles_x), dtype=np.uint16)
    tile_error = np.zeros((tiles_y, tiles_x), dtype=F)
    out = {"rectangles": 0, "pixels_rendered": 0, "passes_run": 0, "checks": []}
    for k in range(max_passes):
        if not active.any():
            break
        for tx0, ty0, tx1, ty1 in plan(active):
            x0, y0, x1, y1 = tx0 * tile, ty0 * tile, min(width, tx1 * tile), min(height, ty1 * tile)
            frame = np.asarray(render(seed + k, x0, y0, x1 - x0, y1 - y0), dtype=F)
            assert frame.shape == (y1 - y0, x1 - x0, 3)
            if k == 0:  # (pass 0 writes, later passes add: ff_render_progressive's rule)
                total[y0:y1, x0:x1] = frame
                even[y0:y1, x0:x1] = frame
            else:
                total[y0:y1, x0:x1] = total[y0:y1, x0:x1] + frame
                if k % 2 == 0:
                    even[y0:y1, x0:x1] = even[y0:y1, x0:x1] + frame
            out["rectangles"] += 1
            out["pixels_rendered"] += (x1 - x0) * (y1 - y0)
        n = k + 1
        tile_passes[active] = n
        out["passes_run"] = n
        if n % 2 or n < min_passes:
            continue
        fresh = tile_errors(total, even, tile, n)
        tile_error[active] = fresh[active]
        with np.errstate(invalid="ignore"):
            below = ~active | (tile_error < threshold)
        before = active.copy()
        stop = before & below
        if guard:
            for ty in range(tiles_y):
                for tx in range(tiles_x):
                    if stop[ty, tx] and not all(below[q] for q in neighbours(tiles_y, tiles_x, ty, tx)):
                        stop[ty, tx] = False
        active = before & ~stop
        out["checks"].append({"n": n, "error": tile_error.copy(), "active_before": before, "stopped": stop.copy()})
    per_pixel = np.repeat(np.repeat(tile_passes, tile, axis=0), tile, axis=1)[:height, :width]
    inv = (F(1.0) / per_pixel.astype(F))[..., None]
    radiance = (total * inv).astype(F)
    out.update({"sum": total, "sum_even": even, "tile_passes": tile_passes, "tile_error": tile_error, "radiance": radiance, "rgb8": to_u8(radiance),
                "passes": per_pixel.astype(np.uint16)})
    return out
