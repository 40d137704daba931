"""Float64 numpy path walker: FF_SHADE_DIFFUSE_PATH and FF_SHADE_DIFFUSE_PATH_NEE of ff_api.h over whole paths (any bounces >= 1, any
spp), under a light table, an environment, albedo textures, rough mirrors and a camera-sampling setting.  Test infrastructure only.

It strings the host twins together the way nee_ref, env_ref, glossy_ref and camera_ref do for one vertex: the camera ray from the ray
matrix (camera_ref.pinhole) or from ff_camera_sample_rays, every closest hit from the `intersect` callable it is given
(Tracer.intersect_rays on the GPU, the CPU oracle's orc_intersect_rays on the host), the light table from ff_light_table, the alias
decisions from the library's float32 tables, the texel from ff_surface_uv and ff_texture_sample, the direction sampled at a rough
mirror from ff_glossy_sample.  Everything else - the scatter directions (the oracle's definition of diffuse, mirror and glass), the
throughput, the light samples, the lobe (glossy_ref.lobe), the MIS weights, the environment lookup and the accumulation - is computed
here in float64 from the text of ff_api.h.  The first vertex is traced here too; ff_gbuffer is not used.

EXCUSED pixels.  Every extension and shadow ray is traced three times, as computed and turned by +-nee_ref.EXCUSE_ANGLE about a
tangent (nee_ref._trace3); a pixel with a ray whose (geometry, triangle) changes under the turn is excused, and so is one with a miss
whose environment texel changes under it, or with a glass vertex whose discrete decision sits within DECISION_EPS of its threshold
(u1 against the Fresnel reflectance F, s2 against 1: float32 and float64 may then take different branches).
A pixel is also excused where an extension ray grazes a SPHERE so closely that the hit's unit normal turns by more than NORMAL_TURN =
100 EXCUSE_ANGLE = 2e-3 under that turn, about either tangent.  Float32 holds a direction to about 1e-7 rad = EXCUSE_ANGLE / 200, so
such a normal - and with it the frame, every cosine and the next ray - differs between two float32 evaluations of the same path by
more than 1e-5, a tenth of RTOL, before the rest of the path amplifies it: the walker's own value is then no reference.  (Measured
on the host: with the ray directions handed to the intersector moved by one float32 ulp, the one such pixel of rough_0.6_nee's first
frame moved by 1.9 allowances and no other pixel by more than 0.8.)  Planes and triangles have one geometric normal each.

TOLERANCE.  The rule of the bounces = 2 references, |got - ref| <= 1e-4 |ref| + 1e-6 per channel (RTOL, ATOL), holds at every depth.
Measured on the CPU (tests/test_path_ref_host.py: the walker with the oracle's intersector against oracle_render, which the GPU suite
pins bit for bit to the kernels; 24x16, spp 1 and 3, the four scenes of that file), the largest deviation of a non-excused pixel, as a
fraction of what the rule allows that pixel, was
    bounces 1: 0 (exact)   bounces 2: 0.0007   bounces 3: 0.0007   bounces 5: 0.0014
(in absolute terms at most 6e-8: the rounding of float32 throughputs and sums), so four times the maximum is within the rule at every
depth - the margin of four stands for the divisions by pdfs the NEE terms add - and the rule is the tolerance everywhere.  At most 0.8 %
of the hit pixels were excused there.  The tolerance was not derived from GPU output."""
import types as _types

import numpy as np

from gpupathtracer_amd import lib
from gpupathtracer_amd import types as T
from nee_ref import EXCUSE_ANGLE, RAY_EPS, KEY_POINT, KEY_SELECT, _tangent, _trace3, _unit, emission_of, frame_key, philox, u24
from glossy_ref import MIN_ALPHA, MIN_COS, lobe
import camera_ref
import env_ref

RTOL, ATOL = 1e-4, 1e-6
DECISION_EPS = 1e-5
NORMAL_TURN = 100.0 * EXCUSE_ANGLE
COUNTERS = ("light_samples_deep", "mis_emitter_hits_deep", "emitter_hits_after_specular", "env_misses_last_segment", "texture_lookups_deep",
            "glossy_deaths_pending_shadow", "refracted_segments")


def within(got, ref):
    """[H, W] mask of the pixels whose channels are all within the tolerance."""
    return np.all(np.abs(got - ref) <= RTOL * np.abs(ref) + ATOL, -1)


def _vec(v):
    return np.array([v.x, v.y, v.z], np.float32).astype(np.float64)


def _materials(scene):
    out = {k: [] for k in ("albedo", "specular", "transmittance", "ior", "shape")}
    for i in range(len(scene)):
        g = scene.geometries[i]
        b = g.m_bxdf.contents
        out["albedo"].append(_vec(b.m_albedo))
        out["specular"].append(_vec(b.m_specularColor))
        out["transmittance"].append(_vec(b.m_transmittanceColor))
        out["ior"].append(float(np.float32(b.m_refractiveIndex)))
        out["shape"].append(g.m_geometryType)
    return {k: np.array(v) for k, v in out.items()}


def _camera_rays(cam, params, sampling, jitter, xs, ys, ss):
    active = sampling is not None and (sampling.pixel_filter == T.PIXEL_BOX or sampling.lens_radius > 0.0)
    if active:  # (the twin applies the BOX rule: the unjittered matrix)
        o, d = lib.camera_sample_rays(cam, sampling, params.width, params.seed, xs, ys, ss, jitter=jitter)
        return o.astype(np.float64), d.astype(np.float64)
    zero = np.zeros(len(xs), np.float32)
    d = camera_ref.pinhole(cam, camera_ref.ray_matrix(cam, jitter), xs, ys, zero, zero)
    o = np.broadcast_to(camera_ref.vec(cam.m_position), d.shape)
    return o.astype(np.float64), d.astype(np.float64)


def _unsteady_normals(intersect, shapes, org, dirn, h, hitm):
    """Indices of the extension rays that graze a SPHERE: the hit's unit normal turns by more than NORMAL_TURN under a turn of the ray
    by EXCUSE_ANGLE about either tangent (or the turned ray leaves the sphere).  Planes and triangles have one normal each."""
    g = np.asarray(h["geom"])
    idx = np.nonzero(hitm & (shapes[np.where(hitm, g, 0)] == T.GEOM_SPHERE))[0]
    if len(idx) == 0:
        return idx
    d = _unit(dirn[idx])
    n0 = _unit(np.asarray(h["normal"])[idx].astype(np.float64))
    out = np.zeros(len(idx), bool)
    for basis in _tangent(d):
        for sgn in (1.0, -1.0):
            k = intersect(org[idx].astype(np.float32), _unit(d + sgn * EXCUSE_ANGLE * basis).astype(np.float32))
            same = (np.asarray(k["hit"]) != 0) & (np.asarray(k["geom"]) == g[idx])
            with np.errstate(invalid="ignore", divide="ignore"):
                turn = np.linalg.norm(_unit(np.asarray(k["normal"]).astype(np.float64)) - n0, axis=-1)
            out |= ~same | ~(turn <= NORMAL_TURN)
    return idx[out]


def walk(intersect, scene, cam, params, *, environment=None, textures=None, roughness=None, sampling=None, jitter=(0.0, 0.0)):
    """One frame in float64: (radiance [H, W, 3], excused [H, W] bool, stats).

    intersect(origins, directions) returns lib.INTERSECT_DTYPE records.  environment = (rgb [h, w, 3], intensity, rotation_deg);
    textures = {geometry: (texels, flags, scale, offset)}; roughness = {geometry: roughness}; sampling an FfCameraSampling; jitter the
    state's pixel jitter.  stats holds the counters of COUNTERS for the frame and "hit", the [H, W] mask of pixels with a sample whose
    camera ray hits something."""
    W, H, spp, bounces = params.width, params.height, params.spp, params.bounces
    assert params.shade_mode in (T.SHADE_DIFFUSE_PATH, T.SHADE_DIFFUSE_PATH_NEE) and bounces >= 1 and spp >= 1
    nee = params.shade_mode == T.SHADE_DIFFUSE_PATH_NEE
    textures, roughness = textures or {}, roughness or {}
    key = frame_key(params.seed)
    shim = _types.SimpleNamespace(intersect_rays=intersect)
    kinds, le = emission_of(scene)
    mat = _materials(scene)
    entries, pdf_area = lib.light_table(scene)
    pdf_area = pdf_area.astype(np.float64)
    n_lights = len(entries["area"])
    alpha_of = np.zeros(len(scene))
    for g, r in roughness.items():
        if kinds[g] == T.BXDF_MIRROR:
            alpha_of[g] = float(np.float32(r) * np.float32(r))
    # the environment: what a miss looks up, and the table the light sample draws from
    env_on = environment is not None
    p_env = 0.0
    if env_on:
        rgb, intensity, rotation_deg = environment
        rgb = np.asarray(rgb, np.float32)
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
    sample_lights = nee and (n_lights > 0 or p_env > 0.0)

    ys, xs, ss = (a.reshape(-1) for a in np.meshgrid(np.arange(H), np.arange(W), np.arange(spp), indexing="ij"))
    N = len(ys)
    gpix_all = ys.astype(np.uint64) * np.uint64(W) + xs.astype(np.uint64)
    L = np.zeros((N, 3))
    bad = np.zeros(N, bool)  # paths with a decision float32 may take differently
    first_hit = np.zeros(N, bool)
    stats = {k: 0 for k in COUNTERS}

    pid = np.arange(N)
    org, dirn = _camera_rays(cam, params, sampling, jitter, xs, ys, ss)
    beta = np.ones((N, 3))
    prev_pdf = np.zeros(N)  # 0: the camera ray, or a mirror / glass bounce (weight 1)
    spec = np.zeros(N, bool)  # the segment leaves a mirror or glass vertex
    for b in range(bounces):
        if len(pid) == 0:
            break
        last = b == bounces - 1
        h, flips = _trace3(shim, org, dirn, _tangent(_unit(dirn))[0])
        bad[pid[flips]] = True
        hitm = (np.asarray(h["hit"]) != 0) & (np.asarray(h["geom"]) >= 0)
        bad[pid[_unsteady_normals(intersect, mat["shape"], org, dirn, h, hitm)]] = True
        if b == 0:
            first_hit[pid[hitm]] = True
        # ---- a miss: the environment, on every segment including the last
        mi = np.nonzero(~hitm)[0]
        if env_on and len(mi):
            wd = _unit(dirn[mi])
            k = texel_index(wd)
            pl = p_env * env_pdf[k]
            pb = prev_pdf[mi]
            wgt = np.where(nee & (pb > 0.0) & (pl > 0.0), pb ** 2 / (pb ** 2 + pl ** 2 + 1e-300), 1.0)
            L[pid[mi]] += beta[mi] * env_le[k] * wgt[:, None]
            tb, sb = _tangent(wd)
            fl = np.zeros(len(mi), bool)
            for basis in (tb, sb):
                for sgn in (1.0, -1.0):
                    fl |= texel_index(_unit(wd + sgn * EXCUSE_ANGLE * basis)) != k
            bad[pid[mi[fl]]] = True
            if last:
                stats["env_misses_last_segment"] += len(mi)
        # ---- hits
        hi = np.nonzero(hitm)[0]
        pid, org, dirn, beta, prev_pdf, spec = pid[hi], org[hi], dirn[hi], beta[hi], prev_pdf[hi], spec[hi]
        g = np.asarray(h["geom"])[hi]
        tri = np.asarray(h["tri"])[hi]
        x32 = np.asarray(h["point"])[hi]
        x = x32.astype(np.float64)
        t_hit = np.asarray(h["t"])[hi].astype(np.float64)
        n = _unit(np.asarray(h["normal"])[hi].astype(np.float64))
        flipped = np.sum(n * dirn, -1) > 0.0
        n = np.where(flipped[:, None], -n, n)
        kind = kinds[g]
        # emitter hits end the path
        em = kind == T.BXDF_EMITTER
        ie = np.nonzero(em)[0]
        if len(ie):
            wgt = np.ones(len(ie))
            pa = pdf_area[g[ie]]
            mis = nee & (prev_pdf[ie] > 0.0) & (pa > 0.0)
            cos_y = np.abs(np.sum(n[ie] * _unit(dirn[ie]), -1))
            with np.errstate(divide="ignore", invalid="ignore"):
                pl = p_area * pa * t_hit[ie] ** 2 / cos_y
                wmis = prev_pdf[ie] ** 2 / (prev_pdf[ie] ** 2 + pl ** 2)
            wgt = np.where(mis, wmis, 1.0)
            L[pid[ie]] += beta[ie] * le[g[ie]] * wgt[:, None]
            if b >= 2:
                stats["mis_emitter_hits_deep"] += int(mis.sum())
            stats["emitter_hits_after_specular"] += int(spec[ie].sum())
        keep = np.nonzero(~em)[0]
        pid, org, dirn, beta, prev_pdf, spec = pid[keep], org[keep], dirn[keep], beta[keep], prev_pdf[keep], spec[keep]
        g, tri, x32, x, n, flipped, kind = g[keep], tri[keep], x32[keep], x[keep], n[keep], flipped[keep], kind[keep]
        if len(pid) == 0:
            break
        glass = kind == T.BXDF_GLASS
        glossy = (kind == T.BXDF_MIRROR) & (alpha_of[g] >= MIN_ALPHA)
        mirror = (kind == T.BXDF_MIRROR) & ~glossy
        diffuse = ~(glass | glossy | mirror)
        # the surface's tint joins the throughput at the hit (not at a glossy or glass one)
        tint = np.where(mirror[:, None], mat["specular"][g], mat["albedo"][g])
        for gi, (texels, flags, scale, offset) in textures.items():
            m = np.nonzero(diffuse & (g == gi))[0]
            if len(m) == 0:
                continue
            uv = lib.surface_uv(scene, gi, x32[m], tri[m] if mat["shape"][gi] == T.GEOM_TRIANGLEMESH else None)
            c = (uv * np.asarray(scale, np.float32) + np.asarray(offset, np.float32)).astype(np.float32)
            tint[m] = (mat["albedo"][gi].astype(np.float32) * lib.texture_sample(texels, c, flags)).astype(np.float64)
            if b >= 1:
                stats["texture_lookups_deep"] += len(m)
        plain = diffuse | mirror
        beta[plain] = beta[plain] * tint[plain]
        if last:
            break
        # ---- the vertex: frame, light sample, scatter
        gpix = gpix_all[pid]
        ctr = (ss[pid].astype(np.uint64) << np.uint64(8)) | np.uint64(b)
        t_basis, s_basis = _tangent(n)
        origin = x + RAY_EPS * n
        to_eye = -_unit(x - org)  # (minus the ray's direction, in float64 from its two ends)
        wo_l = np.stack([np.sum(t_basis * to_eye, -1), np.sum(s_basis * to_eye, -1), np.maximum(np.sum(n * to_eye, -1), MIN_COS)], -1)
        f0 = mat["specular"][g]
        alpha = alpha_of[g]
        ig = np.nonzero(glossy)[0]

        def surface_terms(idx, w):
            """(f cos [k, 3] not times beta, pdf_b [k]) of the world directions w at the vertices idx (diffuse or glossy)."""
            cz = np.sum(n[idx] * w, -1)
            fcos = np.repeat((cz / np.pi)[:, None], 3, 1)  # (beta holds the albedo of a diffuse vertex)
            pb = cz / np.pi
            kk = np.nonzero(glossy[idx])[0]
            for a in np.unique(alpha[idx[kk]]):
                m = kk[alpha[idx[kk]] == a]
                j = idx[m]
                wl = np.stack([np.sum(t_basis[j] * w[m], -1), np.sum(s_basis[j] * w[m], -1), cz[m]], -1)
                f, pdf, _ = lobe(a, f0[j], wo_l[j], wl)
                fcos[m] = f * cz[m][:, None]
                pb[m] = pdf
            return fcos, pb

        pending = np.zeros(len(pid), bool)  # a shadow ray was traced at this vertex
        lit = np.nonzero(diffuse | glossy)[0] if sample_lights else np.zeros(0, np.int64)
        if len(lit):
            a0, a1 = philox(gpix[lit], ctr[lit], key ^ KEY_SELECT)
            q0, q1 = philox(gpix[lit], ctr[lit], key ^ KEY_POINT)
            if 0.0 < p_env < 1.0:
                c0, _ = philox(gpix[lit], ctr[lit], key ^ env_ref.KEY_CHOOSE)
                pick_env = u24(c0) < p_env
            else:
                pick_env = np.full(len(lit), p_env >= 1.0)
            taken = 0
            # the environment's branch
            je = np.nonzero(pick_env)[0]
            if len(je):
                k = ((a0[je] * np.uint64(ew * eh)) >> np.uint64(32)).astype(np.int64)
                k = np.where(u24(a1[je]) < e_ap[k], k, e_alias[k])
                row, col = k // ew, k % ew
                z = z_rows[row] + u24(q0[je]) * (z_rows[row + 1] - z_rows[row])
                phi = (col + u24(q1[je])) * (2.0 * np.pi / ew) + rot
                st = np.sqrt(np.maximum(0.0, 1.0 - z * z))
                wd = np.stack([st * np.sin(phi), z, -st * np.cos(phi)], -1)
                v = lit[je]
                cos_x = np.sum(n[v] * wd, -1)
                pl = p_env * env_pdf[k]
                sel = np.nonzero((cos_x > 0.0) & (pl > 0.0))[0]
                if len(sel):
                    v, wd, k, pl = v[sel], wd[sel], k[sel], pl[sel]
                    hs, fl = _trace3(shim, origin[v], wd, _tangent(wd)[0])
                    bad[pid[v[fl]]] = True
                    pending[v] = True
                    vis = (np.asarray(hs["hit"]) == 0) | (np.asarray(hs["geom"]) < 0)
                    fcos, pb = surface_terms(v, wd)
                    wl = pl ** 2 / (pl ** 2 + pb ** 2)
                    contrib = beta[v] * env_le[k] * fcos * (wl / pl)[:, None]
                    L[pid[v[vis]]] += contrib[vis]
                    taken += int(vis.sum())
            # the light table's branch
            jt = np.nonzero(~pick_env)[0]
            if n_lights > 0 and len(jt):
                k = ((a0[jt] * np.uint64(n_lights)) >> np.uint64(32)).astype(np.int64)
                k = np.where(u24(a1[jt]) < entries["alias_probability"][k].astype(np.float64), k, entries["alias"][k])
                su, sv = u24(q0[jt]), u24(q1[jt])
                is_tri = entries["primitive"][k] >= 0
                r = np.sqrt(su)
                su, sv = np.where(is_tri, r * (1.0 - sv), su), np.where(is_tri, r * sv, sv)
                y = entries["v0"][k].astype(np.float64) + su[:, None] * entries["e1"][k] + sv[:, None] * entries["e2"][k]
                v = lit[jt]
                dv = y - x[v]
                d2 = np.sum(dv * dv, -1)
                wd = dv / np.sqrt(d2)[:, None]
                cos_x = np.sum(n[v] * wd, -1)
                cos_y = np.abs(np.sum(entries["normal"][k].astype(np.float64) * wd, -1))
                sel = np.nonzero((cos_x > 0.0) & (cos_y > 0.0))[0]
                if len(sel):
                    v, wd, k, d2, cos_y = v[sel], wd[sel], k[sel], d2[sel], cos_y[sel]
                    hs, fl = _trace3(shim, origin[v], wd, _tangent(wd)[0])
                    bad[pid[v[fl]]] = True
                    pending[v] = True
                    g_l, p_l = entries["geometry"][k], entries["primitive"][k]
                    vis = (np.asarray(hs["hit"]) != 0) & (np.asarray(hs["geom"]) == g_l) & ((p_l < 0) | (np.asarray(hs["tri"]) == p_l))
                    pl = p_area * pdf_area[g_l] * d2 / cos_y
                    fcos, pb = surface_terms(v, wd)
                    wl = pl ** 2 / (pl ** 2 + pb ** 2)
                    contrib = beta[v] * le[g_l] * fcos * (wl / pl)[:, None]
                    L[pid[v[vis]]] += contrib[vis]
                    taken += int(vis.sum())
            if b >= 1:
                stats["light_samples_deep"] += taken
        # ---- scatter
        r0, r1 = philox(gpix, ctr, key)
        u1 = u24(r0)
        new_dir = np.zeros_like(dirn)
        new_org = origin.copy()
        new_pdf = np.zeros(len(pid))
        alive = np.ones(len(pid), bool)
        # diffuse: the cosine-weighted direction about n^
        theta = 2.0 * np.pi * (r1 >> np.uint64(8)).astype(np.float64) / 2.0 ** 24
        rr = np.sqrt(u1)
        lx, ly, lz = rr * np.cos(theta), rr * np.sin(theta), np.sqrt(np.maximum(0.0, 1.0 - u1))
        wdif = _unit(t_basis * lx[:, None] + s_basis * ly[:, None] + n * lz[:, None])
        new_dir[diffuse] = wdif[diffuse]
        new_pdf[diffuse] = (np.sum(n * wdif, -1) / np.pi)[diffuse]
        # mirror: d - 2 (n . d) n with the facing normal
        nd = np.sum(n * dirn, -1)
        refl = dirn - 2.0 * nd[:, None] * n
        new_dir[mirror] = refl[mirror]
        # glass: the facing side decides entering / leaving; u1 picks reflection with probability F; total internal reflection reflects
        jg = np.nonzero(glass)[0]
        if len(jg):
            ior = mat["ior"][g[jg]]
            eta = np.where(flipped[jg], ior, 1.0 / ior)
            ci = -nd[jg]
            s2 = eta * eta * (1.0 - ci * ci)
            ct = np.sqrt(np.maximum(0.0, 1.0 - s2))
            aa, bq = eta * ci, eta * ct
            with np.errstate(divide="ignore", invalid="ignore"):
                rs, rp = (aa - ct) / (aa + ct), (ci - bq) / (ci + bq)
            fres = 0.5 * (rs * rs + rp * rp)
            tir = ~(s2 < 1.0)
            reflect = tir | (u1[jg] < fres)
            bad[pid[jg[np.abs(s2 - 1.0) < DECISION_EPS]]] = True
            bad[pid[jg[~tir & (np.abs(u1[jg] - fres) < DECISION_EPS)]]] = True
            refr = eta[:, None] * dirn[jg] + (eta * ci - ct)[:, None] * n[jg]
            new_dir[jg] = np.where(reflect[:, None], refl[jg], refr)
            new_org[jg] = np.where(reflect[:, None], origin[jg], x[jg] - RAY_EPS * n[jg])
            beta[jg] = beta[jg] * np.where(reflect[:, None], mat["specular"][g[jg]], mat["transmittance"][g[jg]])
            stats["refracted_segments"] += int((~reflect).sum())
        # rough mirror: the sampler's host twin; a direction on or below the horizon ends the sample
        for a in np.unique(alpha[ig]):
            m = ig[alpha[ig] == a]
            u = np.stack([u1[m], u24(r1[m])], -1).astype(np.float32)
            wi = lib.glossy_sample(a, (1.0, 1.0, 1.0), wo_l[m].astype(np.float32), u)[0].astype(np.float64)
            up = wi[:, 2] > 0.0
            _, _, weight = lobe(a, f0[m], wo_l[m], wi)
            alive[m] = up
            beta[m] = beta[m] * weight
            new_dir[m] = _unit(t_basis[m] * wi[:, 0:1] + s_basis[m] * wi[:, 1:2] + n[m] * wi[:, 2:3])
            new_pdf[m] = surface_terms(m, new_dir[m])[1]  # (the pdf of the unit direction the ray takes, as glossy_ref has it)
            stats["glossy_deaths_pending_shadow"] += int((~up & pending[m]).sum())
        if not nee:
            new_pdf[:] = 0.0  # (every weight is 1)
        spec = mirror | glass
        pid, org, dirn, beta, prev_pdf, spec = pid[alive], new_org[alive], new_dir[alive], beta[alive], new_pdf[alive], spec[alive]

    # accumulation: blocks of samples summed in order, the blocks added in order, times 1 / spp
    Ls = L.reshape(H, W, spp, 3)
    block = 64 * ((spp + 1023) // 1024)
    total = np.zeros((H, W, 3))
    for first in range(0, spp, block):
        acc = np.zeros((H, W, 3))
        for s in range(first, min(spp, first + block)):
            acc = acc + Ls[:, :, s]
        total = total + acc
    stats["hit"] = first_hit.reshape(H, W, spp).any(-1)
    return total * (1.0 / spp), bad.reshape(H, W, spp).any(-1), stats
