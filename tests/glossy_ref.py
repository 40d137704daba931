"""Float64 numpy restatement of the rough-specular lobe (ff_api.h: GGX, height-correlated Smith, Schlick; visible normals by spherical
caps) and the direct lighting (bounces = 2) of FF_SHADE_DIFFUSE_PATH_NEE on scenes with rough mirrors, in the manner of
nee_ref.direct_lighting and env_ref.direct_lighting.

As there, the primary hits come from ff_gbuffer, the light table from ff_light_table, the alias decisions from the library's own
tables, and the visibility of shadow rays and what a BSDF-sampled ray hits from ff_intersect_rays, traced three times with the
+-EXCUSE_ANGLE turn for the excuse mask.  The direction sampled at a glossy vertex comes from the host twin ff_glossy_sample (the
map from u to the direction is ill-conditioned where 1 - z^2 vanishes; tests/test_glossy_host.py tests it on its own); its pdf, its
weight, the lobe under the light sample, the MIS weights and the contributions are computed here in float64."""
import numpy as np

from gpupathtracer_amd import lib, scenes
from gpupathtracer_amd import types as T
from nee_ref import EXCUSE_ANGLE, RAY_EPS, KEY_POINT, KEY_SELECT, _tangent, _trace3, _unit, emission_of, frame_key, philox, u24
import env_ref

MIN_ALPHA = 1e-3
MIN_COS = 1e-6


# ---- the lobe ----------------------------------------------------------------------------------------------------------------

def _lambda(a2, w):
    z = np.maximum(w[..., 2], MIN_COS)
    return (np.sqrt(1.0 + a2 * (w[..., 0] ** 2 + w[..., 1] ** 2) / (z * z)) - 1.0) / 2.0


def lobe(alpha, f0, wo, wi):
    """(f [..., 3], pdf [...], weight [..., 3]) of unit local directions wo, wi [..., 3] in float64: the BRDF not times cosine, the
    solid-angle pdf of wi under the sampler, and f wi.z / pdf = F G2 / G1.  All 0 where wi.z <= 0.  wo.z is clamped to >= 1e-6."""
    wo = np.array(wo, np.float64)
    wi = np.asarray(wi, np.float64)
    wo[..., 2] = np.maximum(wo[..., 2], MIN_COS)
    f0 = np.asarray(f0, np.float64)
    a2 = np.float64(alpha) ** 2
    h = _unit(wo + wi)
    q = a2 * h[..., 2] ** 2 + (h[..., 0] ** 2 + h[..., 1] ** 2)
    D = a2 / (np.pi * q * q)
    lo, li = _lambda(a2, wo), _lambda(a2, wi)
    G1, G2 = 1.0 / (1.0 + lo), 1.0 / (1.0 + lo + li)
    c = np.maximum(np.sum(wo * h, -1), 0.0)
    F = f0 + (1.0 - f0) * ((1.0 - c) ** 5)[..., None]
    up = wi[..., 2] > 0.0
    f = F * (D * G2 / (4.0 * wo[..., 2] * np.maximum(wi[..., 2], MIN_COS)))[..., None]
    pdf = G1 * D / (4.0 * wo[..., 2])
    weight = F * (G2 / G1)[..., None]
    return np.where(up[..., None], f, 0.0), np.where(up, pdf, 0.0), np.where(up[..., None], weight, 0.0)


def half_vector(alpha, wo, u1, u2):
    """The sampler's half vector h [..., 3] for wo [..., 3] and u1, u2 [...] in float64 (h.z >= 0)."""
    wo = np.array(wo, np.float64)
    wo[..., 2] = np.maximum(wo[..., 2], MIN_COS)
    v = _unit(np.stack([alpha * wo[..., 0], alpha * wo[..., 1], wo[..., 2]], -1))
    z = (1.0 - u2) * (1.0 + v[..., 2]) - v[..., 2]
    r = np.sqrt(np.maximum(0.0, 1.0 - z * z))
    c = np.stack([r * np.cos(2.0 * np.pi * u1), r * np.sin(2.0 * np.pi * u1), z], -1)
    hp = c + v
    return _unit(np.stack([alpha * hp[..., 0], alpha * hp[..., 1], np.maximum(hp[..., 2], 0.0)], -1))


def sample(alpha, wo, u1, u2):
    """The sampler in float64: wi [..., 3] = 2 dot(wo, h) h - wo."""
    wo = np.array(wo, np.float64)
    wo[..., 2] = np.maximum(wo[..., 2], MIN_COS)
    h = half_vector(alpha, wo, u1, u2)
    return 2.0 * np.sum(wo * h, -1)[..., None] * h - wo


def directions(cos_z, azimuth):
    """Unit float32 directions (then float64 copies of exactly those) with z = cos_z at the given azimuth."""
    cz = np.asarray(cos_z, np.float64)
    st = np.sqrt(np.maximum(0.0, 1.0 - cz * cz))
    d = np.stack([st * np.cos(azimuth), st * np.sin(azimuth), cz + 0.0 * st], -1)
    return _unit(d).astype(np.float32)


# ---- scenes ------------------------------------------------------------------------------------------------------------------

def with_mirror(scene, index, specular=(0.9, 0.8, 0.7)):
    """A copy of `scene` whose geometry `index` carries a FF_BXDF_MIRROR bxdf with that m_specularColor."""
    s = scenes.Scene()
    s._specs = list(scene._specs)
    s._specs[index] = s._specs[index][:5] + (scenes.make_bxdf(T.BXDF_MIRROR, specular=specular),)
    return s.finalize()


def lone_sphere_scene(specular=(1.0, 1.0, 1.0), radius=1.0):
    """One mirror sphere at the origin and nothing else (the furnace and the environment tests)."""
    s = scenes.Scene()
    s.add_sphere(radius, (0.0, 0.0, 0.0), (0, 0, 0), (1, 1, 1), scenes.make_bxdf(T.BXDF_MIRROR, specular=specular))
    return s.finalize()


def sphere_on_floor_scene():
    """A mirror sphere above a diffuse floor plane, open to the environment."""
    s = scenes.Scene()
    s.add_sphere(1.0, (0.0, 0.0, 0.0), (0, 0, 0), (1, 1, 1), scenes.make_bxdf(T.BXDF_MIRROR, specular=(0.9, 0.85, 0.6)))
    s.add_plane((0, -1.0, 0), (90, 0, 0), (8, 8, 8), scenes.make_bxdf(T.BXDF_DIFFUSE, albedo=(0.7, 0.7, 0.7)))
    return s.finalize()


# ---- direct lighting ---------------------------------------------------------------------------------------------------------

def direct_lighting(tracer, scene, cam, params, roughness, env=None):
    """FF_SHADE_DIFFUSE_PATH_NEE at bounces = 2 in float64 on `scene` with the bindings `roughness` ({geometry: roughness}) and,
    optionally, the environment env = (rgb, intensity, rotation_deg): (radiance [H, W, 3], hit mask, excused mask).  Pixels whose
    camera ray misses are left at 0.  Every mirror a camera ray sees must be bound with alpha >= 1e-3."""
    assert params.bounces == 2
    W, H, spp = params.width, params.height, params.spp
    key = frame_key(params.seed)
    gb = tracer.gbuffer(cam, params)
    ids = gb["ids"]
    hit = ids[..., 0] >= 0
    kinds, le = emission_of(scene)
    entries, pdf_area = lib.light_table(scene)
    n_lights = len(entries["area"])
    alpha_of = np.zeros(len(scene))
    for g, r in roughness.items():
        alpha_of[g] = float(np.float32(r) * np.float32(r))
    p_env = 0.0
    if env is not None:
        rgb, intensity, rotation_deg = env
        eh, ew = rgb.shape[:2]
        env_le = env_ref.radiance(rgb, intensity).astype(np.float64).reshape(-1, 3)
        env_pdf = env_ref.table(rgb)[1].ravel()
        etab = lib.environment_table(rgb)
        e_ap = etab["alias_probability"].ravel().astype(np.float64)
        e_alias = etab["alias"].ravel()
        z_rows = np.cos(np.pi * np.arange(eh + 1) / eh)
        rot = np.radians(rotation_deg % 360.0)
        if env_pdf.max() > 0.0:
            p_env = 0.5 if n_lights > 0 else 1.0

        def texel_index(d):
            r, c = env_ref.texel_of(d, ew, eh, rotation_deg)
            return r * ew + c
    p_area = 1.0 - p_env
    out = np.zeros((H, W, 3), np.float64)
    excused = np.zeros((H, W), bool)
    ys, xs = np.nonzero(hit)
    g0 = ids[ys, xs, 0]
    emit = kinds[g0] == T.BXDF_EMITTER
    out[ys[emit], xs[emit]] += le[g0[emit]]
    assert not np.any((kinds[g0] == T.BXDF_MIRROR) & (alpha_of[g0] < MIN_ALPHA)), "a perfect mirror in view"
    assert not np.any(kinds[g0] == T.BXDF_GLASS)
    sel = ~emit
    ys, xs, g0 = ys[sel], xs[sel], g0[sel]
    if len(ys) == 0:
        return out, hit, excused
    gl = kinds[g0] == T.BXDF_MIRROR
    alpha = alpha_of[g0]
    tint = gb["albedo"][ys, xs].astype(np.float64)  # m_albedo, or m_specularColor = F0 of a mirror
    x = gb["position"][ys, xs].astype(np.float64)
    n = _unit(gb["normal"][ys, xs].astype(np.float64))
    cam_pos = np.array([cam.m_position.x, cam.m_position.y, cam.m_position.z], np.float64)
    n = np.where((np.sum(n * (x - cam_pos), -1) > 0.0)[:, None], -n, n)
    gpix = ys.astype(np.uint64) * np.uint64(W) + xs.astype(np.uint64)
    t_basis, s_basis = _tangent(n)
    origin = x + RAY_EPS * n
    to_eye = -_unit(x - cam_pos)
    wo_l = np.stack([np.sum(t_basis * to_eye, -1), np.sum(s_basis * to_eye, -1), np.maximum(np.sum(n * to_eye, -1), MIN_COS)], -1)
    ig = np.nonzero(gl)[0]
    acc = np.zeros((len(ys), 3), np.float64)

    def to_local(w):
        return np.stack([np.sum(t_basis * w, -1), np.sum(s_basis * w, -1), np.sum(n * w, -1)], -1)

    def surface_terms(idx, w):
        """(f cos [k, 3], pdf_b [k]) of the world directions w [k, 3] at the vertices idx."""
        cz = np.sum(n[idx] * w, -1)
        fcos = tint[idx] * (cz / np.pi)[:, None]
        pb = cz / np.pi
        k = np.nonzero(gl[idx])[0]
        for a in np.unique(alpha[idx[k]]):  # (one lobe call per alpha value)
            m = k[alpha[idx[k]] == a]
            j = idx[m]
            wl = np.stack([np.sum(t_basis[j] * w[m], -1), np.sum(s_basis[j] * w[m], -1), cz[m]], -1)
            f, pdf, _ = lobe(a, np.zeros(3), wo_l[j], wl)  # F0 per vertex: Schlick is affine in F0
            f1, _, _ = lobe(a, np.ones(3), wo_l[j], wl)
            fcos[m] = (f + tint[j] * (f1 - f)) * cz[m][:, None]
            pb[m] = pdf
        return fcos, pb

    for s in range(spp):
        ctr = np.full(len(ys), (s << 8) | 0, np.uint64)
        r0, r1 = philox(gpix, ctr, key)
        # BSDF sample: cosine-weighted about n^ at a diffuse vertex, the lobe's sampler (the host twin) at a glossy one
        u1 = u24(r0)
        theta = 2.0 * np.pi * (r1 >> np.uint64(8)).astype(np.float64) / 2.0 ** 24
        rr = np.sqrt(u1)
        local = np.stack([rr * np.cos(theta), rr * np.sin(theta), np.sqrt(np.maximum(0.0, 1.0 - u1))], -1)
        beta = tint.copy()
        alive = np.ones(len(ys), bool)
        for a in np.unique(alpha[ig]):
            m = ig[alpha[ig] == a]
            u = np.stack([u24(r0[m]), u24(r1[m])], -1).astype(np.float32)
            wi, _, _ = lib.glossy_sample(a, (1.0, 1.0, 1.0), wo_l[m].astype(np.float32), u)
            local[m] = wi.astype(np.float64)
            alive[m] = wi[:, 2] > 0.0
            _, _, w0 = lobe(a, np.zeros(3), wo_l[m], local[m])
            _, _, w1 = lobe(a, np.ones(3), wo_l[m], local[m])
            beta[m] = w0 + tint[m] * (w1 - w0)
        wdir = _unit(t_basis * local[:, 0:1] + s_basis * local[:, 1:2] + n * local[:, 2:3])
        ia = np.nonzero(alive)[0]
        _, pb_all = surface_terms(ia, wdir[ia])
        hb, flip_b = _trace3(tracer, origin[ia], wdir[ia], t_basis[ia])
        gb_hit = np.asarray(hb["geom"])
        for j in np.nonzero(gb_hit >= 0)[0]:
            g, i = gb_hit[j], ia[j]
            if kinds[g] != T.BXDF_EMITTER:
                continue
            w = 1.0
            if pdf_area[g] > 0.0:
                ny = _unit(np.array(hb["normal"][j], np.float64))
                cos_y = abs(float(np.dot(ny, wdir[i])))
                pl = p_area * float(pdf_area[g]) * float(hb["t"][j]) ** 2 / cos_y
                w = pb_all[j] ** 2 / (pb_all[j] ** 2 + pl ** 2)
            acc[i] += beta[i] * le[g] * w
        excused[ys[ia[flip_b]], xs[ia[flip_b]]] = True
        if env is not None:
            mj = np.nonzero(gb_hit < 0)[0]
            if len(mj):
                mi = ia[mj]
                k = texel_index(wdir[mi])
                pl = p_env * env_pdf[k]
                w = np.where(pl > 0.0, pb_all[mj] ** 2 / (pb_all[mj] ** 2 + pl ** 2), 1.0)
                acc[mi] += beta[mi] * env_le[k] * w[:, None]
                fl = np.zeros(len(mi), bool)
                for basis in (t_basis[mi], s_basis[mi]):
                    for sgn in (1.0, -1.0):
                        fl |= texel_index(_unit(wdir[mi] + sgn * EXCUSE_ANGLE * basis)) != k
                excused[ys[mi[fl]], xs[mi[fl]]] = True
        if n_lights == 0 and p_env == 0.0:
            continue
        # light sample: the environment or the light table, at diffuse and glossy vertices alike
        a0, a1 = philox(gpix, ctr, key ^ KEY_SELECT)
        q0, q1 = philox(gpix, ctr, key ^ KEY_POINT)
        if 0.0 < p_env < 1.0:
            c0, _ = philox(gpix, ctr, key ^ env_ref.KEY_CHOOSE)
            pick_env = u24(c0) < p_env
        else:
            pick_env = np.full(len(ys), p_env >= 1.0)
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
            idx = np.nonzero((cos_x > 0.0) & (pl > 0.0))[0]
            if len(idx):
                t_sh, _ = _tangent(wd[idx])
                hs, flip_s = _trace3(tracer, origin[ie[idx]], wd[idx], t_sh)
                vis = np.asarray(hs["geom"]) < 0
                fcos, pbl = surface_terms(ie[idx], wd[idx])
                wl = pl[idx] ** 2 / (pl[idx] ** 2 + pbl ** 2)
                contrib = env_le[k[idx]] * fcos * (wl / pl[idx])[:, None]
                acc[ie[idx[vis]]] += contrib[vis]
                excused[ys[ie[idx[flip_s]]], xs[ie[idx[flip_s]]]] = True
        it = np.nonzero(~pick_env)[0]
        if n_lights == 0 or len(it) == 0:
            continue
        k = ((a0[it] * np.uint64(n_lights)) >> np.uint64(32)).astype(np.int64)
        keep = u24(a1[it]) < entries["alias_probability"][k].astype(np.float64)
        k = np.where(keep, k, entries["alias"][k])
        su, sv = u24(q0[it]), u24(q1[it])
        tri = entries["primitive"][k] >= 0
        r = np.sqrt(su)
        su, sv = np.where(tri, r * (1.0 - sv), su), np.where(tri, r * sv, sv)
        y = entries["v0"][k].astype(np.float64) + su[:, None] * entries["e1"][k] + sv[:, None] * entries["e2"][k]
        dv = y - x[it]
        d2 = np.sum(dv * dv, -1)
        w_dir = dv / np.sqrt(d2)[:, None]
        cos_x = np.sum(n[it] * w_dir, -1)
        cos_y = np.abs(np.sum(entries["normal"][k].astype(np.float64) * w_dir, -1))
        idx = np.nonzero((cos_x > 0.0) & (cos_y > 0.0))[0]
        if len(idx) == 0:
            continue
        t_sh, _ = _tangent(w_dir[idx])
        hs, flip_s = _trace3(tracer, origin[it[idx]], w_dir[idx], t_sh)
        g_l = entries["geometry"][k[idx]]
        p_l = entries["primitive"][k[idx]]
        vis = (np.asarray(hs["geom"]) == g_l) & ((p_l < 0) | (np.asarray(hs["tri"]) == p_l))
        pl = p_area * pdf_area[g_l].astype(np.float64) * d2[idx] / cos_y[idx]
        fcos, pbl = surface_terms(it[idx], w_dir[idx])
        wl = pl ** 2 / (pl ** 2 + pbl ** 2)
        contrib = le[g_l] * fcos * (wl / pl)[:, None]
        acc[it[idx[vis]]] += contrib[vis]
        excused[ys[it[idx[flip_s]]], xs[it[idx[flip_s]]]] = True
    out[ys, xs] += acc / spp
    out[~hit] = 0.0
    return out, hit, excused
