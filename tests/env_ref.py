"""Float64 numpy reference for the environment light (ff_api.h): the mapping, the sampling table, an RGBE writer for .hdr test
files, and the direct lighting (bounces = 2) of FF_SHADE_DIFFUSE_PATH_NEE under an environment, in the pattern of
nee_ref.direct_lighting.

As there, the primary hits come from ff_gbuffer, the light table from ff_light_table, the alias decisions from the library's own
tables (ff_light_table, ff_environment_table: float32, as the kernel compares them), and the visibility of shadow rays and what a
BSDF-sampled ray hits from ff_intersect_rays.  Everything else is computed here in float64.  A pixel is EXCUSED when one of its
rays changes its answer - the geometry it hits, or the texel a missing ray looks up - under a turn of EXCUSE_ANGLE radians."""
import numpy as np

from gpupathtracer_amd import lib
from gpupathtracer_amd import types as T
from nee_ref import EXCUSE_ANGLE, RAY_EPS, KEY_POINT, KEY_SELECT, _tangent, _trace3, _unit, emission_of, frame_key, philox, u24

KEY_CHOOSE = 0x3C6EF372
LUM = np.array([0.2126, 0.7152, 0.0722])


# ---- mapping and table ------------------------------------------------------------------------------------------------------

def texel_of(dirs, width, height, rotation_deg=0.0):
    """(row, column) of the texel each unit direction [..., 3] looks up (float64)."""
    d = np.asarray(dirs, np.float64)
    phi = (np.arctan2(d[..., 0], -d[..., 2]) - np.radians(rotation_deg % 360.0)) % (2.0 * np.pi)
    theta = np.arccos(np.clip(d[..., 1], -1.0, 1.0))
    c = np.minimum(np.floor(phi / (2.0 * np.pi) * width).astype(np.int64), width - 1)
    r = np.minimum(np.floor(theta / np.pi * height).astype(np.int64), height - 1)
    return r, c


def solid_angles(width, height):
    """Omega_r per row (float64 [H])."""
    z = np.cos(np.pi * np.arange(height + 1) / height)
    return (2.0 * np.pi / width) * (z[:-1] - z[1:])


def table(rgb):
    """(p [H, W], pdf [H, W]) in float64: p = lum Omega / sum, pdf = p / Omega (all 0 for a black map)."""
    rgb = np.asarray(rgb, np.float64)
    h, w = rgb.shape[:2]
    om = solid_angles(w, h)[:, None]
    wgt = (rgb @ LUM) * om
    s = wgt.sum()
    if not s > 0.0:
        return np.zeros((h, w)), np.zeros((h, w))
    p = wgt / s
    return p, p / om


def alias_probabilities(tab):
    """The probability each texel is drawn with under an alias table (ff_environment_table's), in float64."""
    ap = tab["alias_probability"].astype(np.float64).ravel()
    al = tab["alias"].ravel()
    n = ap.size
    out = ap / n
    np.add.at(out, al, (1.0 - ap) / n)
    return out.reshape(tab["alias"].shape)


def radiance(rgb, intensity):
    """What a ray that looks up a texel adds (times beta): intensity x texel in float32, as ff_set_environment stores it."""
    return np.float32(intensity) * np.asarray(rgb, np.float32)


# ---- Radiance RGBE files ------------------------------------------------------------------------------------------------------

def to_rgbe(rgb):
    """float [H, W, 3] -> uint8 [H, W, 4]: mantissas and the shared exponent, m = floor(v / 2^(e - 136))."""
    rgb = np.asarray(rgb, np.float64)
    mx = rgb.max(-1)
    out = np.zeros(rgb.shape[:2] + (4,), np.uint8)
    nz = mx >= 1e-32
    _, e = np.frexp(mx[nz])  # mx = f 2^e, 0.5 <= f < 1
    scale = np.ldexp(1.0, 8 - e)
    out[nz, :3] = np.clip(np.floor(rgb[nz] * scale[:, None]), 0, 255).astype(np.uint8)
    out[nz, 3] = (e + 128).astype(np.uint8)
    return out


def decode_rgbe(rgbe):
    """uint8 [H, W, 4] -> float32 [H, W, 3] as ff_load_hdr decodes it: m 2^(e - 136), 0 for e = 0."""
    q = np.asarray(rgbe)
    f = np.where(q[..., 3] == 0, 0.0, np.ldexp(1.0, q[..., 3].astype(np.int64) - 136))
    return (q[..., :3].astype(np.float64) * f[..., None]).astype(np.float32)


def _rle_channel(vals):
    out = bytearray()
    i, n = 0, len(vals)
    while i < n:
        run = 1
        while i + run < n and run < 127 and vals[i + run] == vals[i]:
            run += 1
        if run >= 3:
            out += bytes([128 + run, vals[i]])
            i += run
            continue
        j = i
        while j < n and j - i < 128 and not (j + 2 < n and vals[j] == vals[j + 1] == vals[j + 2]):
            j += 1
        out += bytes([j - i]) + bytes(vals[i:j])
        i = j
    return bytes(out)


def hdr_bytes(rgbe, rle=True, header=b"#?RADIANCE\nFORMAT=32-bit_rle_rgbe\nEXPOSURE=1.0\n\n"):
    """The .hdr file of an RGBE array: flat scanlines, or new-style run-length encoded ones (rle; widths 8..32767)."""
    h, w = rgbe.shape[:2]
    out = bytearray(header + b"-Y %d +X %d\n" % (h, w))
    for y in range(h):
        row = rgbe[y]
        if rle and 8 <= w <= 0x7FFF:
            out += bytes([2, 2, w >> 8, w & 255])
            for ch in range(4):
                out += _rle_channel(bytes(row[:, ch]))
        else:
            out += row.tobytes()
    return bytes(out)


# ---- direct lighting ---------------------------------------------------------------------------------------------------------

def direct_lighting(tracer, scene, cam, params, rgb, intensity=1.0, rotation_deg=0.0):
    """FF_SHADE_DIFFUSE_PATH_NEE at bounces = 2 under the environment `rgb` in float64: (radiance [H, W, 3], hit mask [H, W],
    excused mask [H, W]).  Pixels whose camera ray misses are left at 0 (test them with a direct view)."""
    assert params.bounces == 2
    W, H, spp = params.width, params.height, params.spp
    eh, ew = rgb.shape[:2]
    key = frame_key(params.seed)
    gb = tracer.gbuffer(cam, params)
    ids = gb["ids"]
    hit = ids[..., 0] >= 0
    kinds, le = emission_of(scene)
    entries, pdf_area = lib.light_table(scene)
    n_lights = len(entries["area"])
    env_le = radiance(rgb, intensity).astype(np.float64).reshape(-1, 3)
    _, env_pdf = table(rgb)
    env_pdf = env_pdf.ravel()
    etab = lib.environment_table(rgb)
    e_ap = etab["alias_probability"].ravel().astype(np.float64)
    e_alias = etab["alias"].ravel()
    z_rows = np.cos(np.pi * np.arange(eh + 1) / eh)
    rot = np.radians(rotation_deg % 360.0)
    sampled = env_pdf.max() > 0.0
    p_env = 0.0 if not sampled else (0.5 if n_lights > 0 else 1.0)
    p_area = 1.0 - p_env
    out = np.zeros((H, W, 3), np.float64)
    excused = np.zeros((H, W), bool)
    ys, xs = np.nonzero(hit)
    g0 = ids[ys, xs, 0]
    emit = kinds[g0] == T.BXDF_EMITTER
    out[ys[emit], xs[emit]] += le[g0[emit]]
    sel = kinds[g0] == T.BXDF_DIFFUSE
    ys, xs = ys[sel], xs[sel]
    if len(ys) == 0:
        return out, hit, excused
    beta = gb["albedo"][ys, xs].astype(np.float64)
    x = gb["position"][ys, xs].astype(np.float64)
    n = _unit(gb["normal"][ys, xs].astype(np.float64))
    cam_pos = np.array([cam.m_position.x, cam.m_position.y, cam.m_position.z], np.float64)
    n = np.where((np.sum(n * (x - cam_pos), -1) > 0.0)[:, None], -n, n)
    gpix = ys.astype(np.uint64) * np.uint64(W) + xs.astype(np.uint64)
    t_basis, s_basis = _tangent(n)
    origin = x + RAY_EPS * n
    acc = np.zeros((len(ys), 3), np.float64)

    def texel_index(d):
        r, c = texel_of(d, ew, eh, rotation_deg)
        return r * ew + c

    for s in range(spp):
        ctr = np.full(len(ys), (s << 8) | 0, np.uint64)
        # BSDF sample: cosine-weighted about n^, then an emitter, the environment or nothing
        r0, r1 = philox(gpix, ctr, key)
        u1 = u24(r0)
        theta = 2.0 * np.pi * (r1 >> np.uint64(8)).astype(np.float64) / 2.0 ** 24
        rr = np.sqrt(u1)
        lx, ly, lz = rr * np.cos(theta), rr * np.sin(theta), np.sqrt(np.maximum(0.0, 1.0 - u1))
        wo = _unit(t_basis * lx[:, None] + s_basis * ly[:, None] + n * lz[:, None])
        hb, flip_b = _trace3(tracer, origin, wo, t_basis)
        gb_hit = np.asarray(hb["geom"])
        pb = np.sum(n * wo, -1) / np.pi
        for i in np.nonzero(gb_hit >= 0)[0]:
            g = gb_hit[i]
            if kinds[g] != T.BXDF_EMITTER:
                continue
            w = 1.0
            if pdf_area[g] > 0.0:
                ny = _unit(np.array(hb["normal"][i], np.float64))
                cos_y = abs(float(np.dot(ny, wo[i])))
                pl = p_area * float(pdf_area[g]) * float(hb["t"][i]) ** 2 / cos_y
                w = pb[i] ** 2 / (pb[i] ** 2 + pl ** 2)
            acc[i] += beta[i] * le[g] * w
        miss = np.nonzero(gb_hit < 0)[0]
        if len(miss):
            k = texel_index(wo[miss])
            pl = p_env * env_pdf[k]
            w = np.where(pl > 0.0, pb[miss] ** 2 / (pb[miss] ** 2 + pl ** 2), 1.0)
            acc[miss] += beta[miss] * env_le[k] * w[:, None]
            # a direction on a texel boundary may look up its neighbour in float32
            tb = t_basis[miss]
            kp, km = texel_index(_unit(wo[miss] + EXCUSE_ANGLE * tb)), texel_index(_unit(wo[miss] - EXCUSE_ANGLE * tb))
            sb = s_basis[miss]
            kq, kr = texel_index(_unit(wo[miss] + EXCUSE_ANGLE * sb)), texel_index(_unit(wo[miss] - EXCUSE_ANGLE * sb))
            fl = (kp != k) | (km != k) | (kq != k) | (kr != k)
            excused[ys[miss[fl]], xs[miss[fl]]] = True
        excused[ys[flip_b], xs[flip_b]] = True
        if n_lights == 0 and p_env == 0.0:
            continue
        # light sample: the environment or the light table
        a0, a1 = philox(gpix, ctr, key ^ KEY_SELECT)
        q0, q1 = philox(gpix, ctr, key ^ KEY_POINT)
        if 0.0 < p_env < 1.0:
            c0, _ = philox(gpix, ctr, key ^ KEY_CHOOSE)
            pick_env = u24(c0) < p_env
        else:
            pick_env = np.full(len(ys), p_env >= 1.0)
        # environment branch
        ie = np.nonzero(pick_env)[0]
        if len(ie):
            k = ((a0[ie] * np.uint64(ew * eh)) >> np.uint64(32)).astype(np.int64)
            keep = u24(a1[ie]) < e_ap[k]
            k = np.where(keep, k, e_alias[k])
            row, col = k // ew, k % ew
            z = z_rows[row] + u24(q0[ie]) * (z_rows[row + 1] - z_rows[row])
            phi = (col + u24(q1[ie])) * (2.0 * np.pi / ew) + rot
            st = np.sqrt(np.maximum(0.0, 1.0 - z * z))
            wd = np.stack([st * np.sin(phi), z, -st * np.cos(phi)], -1)
            cos_x = np.sum(n[ie] * wd, -1)
            pl = p_env * env_pdf[k]
            ok = (cos_x > 0.0) & (pl > 0.0)
            idx = np.nonzero(ok)[0]
            if len(idx):
                t_sh, _ = _tangent(wd[idx])
                hs, flip_s = _trace3(tracer, origin[ie[idx]], wd[idx], t_sh)
                vis = np.asarray(hs["geom"]) < 0
                pbl = cos_x[idx] / np.pi
                wl = pl[idx] ** 2 / (pl[idx] ** 2 + pbl ** 2)
                contrib = beta[ie[idx]] * env_le[k[idx]] * (pbl * wl / pl[idx])[:, None]
                acc[ie[idx[vis]]] += contrib[vis]
                excused[ys[ie[idx[flip_s]]], xs[ie[idx[flip_s]]]] = True
        # light table branch (nee_ref's, with pdf_l times 1 - p_env)
        ia = np.nonzero(~pick_env)[0]
        if n_lights == 0 or len(ia) == 0:
            continue
        k = ((a0[ia] * np.uint64(n_lights)) >> np.uint64(32)).astype(np.int64)
        keep = u24(a1[ia]) < entries["alias_probability"][k].astype(np.float64)
        k = np.where(keep, k, entries["alias"][k])
        su, sv = u24(q0[ia]), u24(q1[ia])
        tri = entries["primitive"][k] >= 0
        r = np.sqrt(su)
        su, sv = np.where(tri, r * (1.0 - sv), su), np.where(tri, r * sv, sv)
        y = entries["v0"][k].astype(np.float64) + su[:, None] * entries["e1"][k] + sv[:, None] * entries["e2"][k]
        dv = y - x[ia]
        d2 = np.sum(dv * dv, -1)
        w_dir = dv / np.sqrt(d2)[:, None]
        cos_x = np.sum(n[ia] * w_dir, -1)
        cos_y = np.abs(np.sum(entries["normal"][k].astype(np.float64) * w_dir, -1))
        idx = np.nonzero((cos_x > 0.0) & (cos_y > 0.0))[0]
        if len(idx) == 0:
            continue
        t_sh, _ = _tangent(w_dir[idx])
        hs, flip_s = _trace3(tracer, origin[ia[idx]], w_dir[idx], t_sh)
        g_l = entries["geometry"][k[idx]]
        p_l = entries["primitive"][k[idx]]
        vis = (np.asarray(hs["geom"]) == g_l) & ((p_l < 0) | (np.asarray(hs["tri"]) == p_l))
        pl = p_area * pdf_area[g_l].astype(np.float64) * d2[idx] / cos_y[idx]
        pbl = cos_x[idx] / np.pi
        wl = pl ** 2 / (pl ** 2 + pbl ** 2)
        contrib = beta[ia[idx]] * le[g_l] * (pbl * wl / pl)[:, None]
        acc[ia[idx[vis]]] += contrib[vis]
        excused[ys[ia[idx[flip_s]]], xs[ia[idx[flip_s]]]] = True
    out[ys, xs] += acc / spp
    out[~hit] = 0.0
    return out, hit, excused
