"""Float32 numpy restatement of the per-sample camera ray (ff_set_camera_sampling), the estimator of ff_api.h: every operation in
float32, in the order the header parenthesises it, no fused multiply-add (numpy has none).  1 / x and sqrt in numpy float32 are
correctly rounded, as the library's are.  The Philox streams, u24 and the frame key are nee_ref's."""
import ctypes as C

import numpy as np

from gpupathtracer_amd import lib
from gpupathtracer_amd import types as T
import nee_ref

KEY_PIXEL = 0xA54FF53A
KEY_LENS = 0x510E527F
MIN_COS = np.float32(1e-6)
F = np.float32


def ray_matrix(cam, jitter=(0.0, 0.0)):
    """The library's own ray matrix (ff_camera_ray_matrix_jittered; jitter 0 0 is ff_camera_ray_matrix) as float32 [4 cols, 4 rows]."""
    m = lib.camera_ray_matrix_jittered(cam, float(jitter[0]), float(jitter[1]))
    return np.array(list(m.m), np.float32).reshape(4, 4)


def vec(v):
    return np.array([v.x, v.y, v.z], np.float32)


def dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def sincos_turn(k24):
    """ff_glossy.h glossy_sincos_turn on uint64 arrays of 24-bit integers: (sin, cos) of 2 pi k / 2^24 in float32."""
    k24 = np.asarray(k24, np.uint64)
    octant = (k24 >> np.uint64(21)) & np.uint64(7)
    f = k24 & np.uint64(0x1FFFFF)
    mm = np.where((octant & np.uint64(1)) != 0, np.uint64(0x200000) - f, f)
    a = mm.astype(np.float32) * F(3.7450704e-07)
    a2 = a * a
    sp = F(-1.9841270e-04) + a2 * F(2.7557319e-06)
    sp = F(8.3333333e-03) + a2 * sp
    sp = F(-1.6666667e-01) + a2 * sp
    s = a + (a * a2) * sp
    cp = F(-1.3888889e-03) + a2 * F(2.4801587e-05)
    cp = F(4.1666667e-02) + a2 * cp
    cp = F(-0.5) + a2 * cp
    c = F(1.0) + a2 * cp
    swap = ((octant + np.uint64(1)) & np.uint64(2)) != 0
    sn = np.where(swap, c, s)
    cs = np.where(swap, s, c)
    sn = np.where(octant >= 4, -sn, sn)
    cs = np.where((octant >= 2) & (octant <= 5), -cs, cs)
    return sn.astype(np.float32), cs.astype(np.float32)


def pixel_offsets(sampling, width, seed, xs, ys, samples):
    """(fx, fy) float32 of every sample: 0 under CORNER, the box stream's u24 pair under BOX."""
    xs = np.asarray(xs, np.uint64)
    if sampling is None or sampling.pixel_filter != T.PIXEL_BOX:
        return np.zeros(xs.shape, np.float32), np.zeros(xs.shape, np.float32)
    gpix = np.asarray(ys, np.uint64) * np.uint64(width) + xs
    ctr = np.asarray(samples, np.uint64) << np.uint64(8)
    a0, a1 = nee_ref.philox(gpix, ctr, nee_ref.frame_key(seed) ^ KEY_PIXEL)
    return nee_ref.u24(a0).astype(np.float32), nee_ref.u24(a1).astype(np.float32)


def pinhole(cam, m, xs, ys, fx, fy):
    """primary_ray's arithmetic through (x + fx, y + fy): unit directions float32 [n, 3]."""
    sw, sh, far = F(cam.m_screenWidth), F(cam.m_screenHeight), F(cam.m_farClip)
    px = ((np.asarray(xs).astype(np.float32) + fx) / sw) * F(2.0) - F(1.0)
    py = F(1.0) - ((np.asarray(ys).astype(np.float32) + fy) / sh) * F(2.0)
    v0, v1, v2, v3 = px * far, py * far, F(1.0) * far, F(1.0) * far
    w = np.stack([(m[0, k] * v0 + m[1, k] * v1) + (m[2, k] * v2 + m[3, k] * v3) for k in range(3)], -1).astype(np.float32)
    dd = w - vec(cam.m_position)
    inv = F(1.0) / np.sqrt(dot(dd, dd))
    return (dd * inv[..., None]).astype(np.float32)


def sample_rays(cam, sampling, width, seed, xs, ys, samples, jitter=(0.0, 0.0)):
    """(origins, directions) float32 [n, 3]: ff_camera_sample_rays restated."""
    xs, ys, samples = (np.asarray(a, np.int64).reshape(-1) for a in (xs, ys, samples))
    box = sampling is not None and sampling.pixel_filter == T.PIXEL_BOX
    m = ray_matrix(cam) if box else ray_matrix(cam, jitter)
    fx, fy = pixel_offsets(sampling, width, seed, xs, ys, samples)
    d = pinhole(cam, m, xs, ys, fx, fy)
    o = np.broadcast_to(vec(cam.m_position), d.shape).astype(np.float32).copy()
    radius = F(0.0) if sampling is None else F(sampling.lens_radius)
    if not radius > 0:
        return o, d
    fwd, right, up = vec(cam.m_forward), vec(cam.m_right), vec(cam.m_up)
    c = dot(d, fwd)
    lens = c > MIN_COS
    with np.errstate(divide="ignore", over="ignore", invalid="ignore"):
        t = F(sampling.focus_distance) * (F(1.0) / c)
        focus = o + d * t[..., None]
        gpix = ys.astype(np.uint64) * np.uint64(width) + xs.astype(np.uint64)
        l0, l1 = nee_ref.philox(gpix, samples.astype(np.uint64) << np.uint64(8), nee_ref.frame_key(seed) ^ KEY_LENS)
        sn, cs = sincos_turn(l0 >> np.uint64(8))
        rho = radius * np.sqrt(nee_ref.u24(l1).astype(np.float32))
        a, b = rho * cs, rho * sn
        o2 = o + (a[..., None] * right + b[..., None] * up)
        e = focus - o2
        inv = F(1.0) / np.sqrt(dot(e, e))
        d2 = e * inv[..., None]
    o = np.where(lens[..., None], o2, o).astype(np.float32)
    d = np.where(lens[..., None], d2, d).astype(np.float32)
    return o, d


def frame_rays(cam, sampling, width, height, seed, spp, jitter=(0.0, 0.0), twin=True):
    """Every sample's ray of a width x height frame, from the host twin (twin=True) or from this file: origins and directions
    float32 [spp, H, W, 3]."""
    ys, xs, ss = np.meshgrid(np.arange(height), np.arange(width), np.arange(spp), indexing="ij")
    fn = lib.camera_sample_rays if twin else sample_rays
    o, d = fn(cam, sampling, width, seed, xs.reshape(-1), ys.reshape(-1), ss.reshape(-1), jitter=jitter)
    shape = (height, width, spp, 3)
    return np.moveaxis(o.reshape(shape), 2, 0), np.moveaxis(d.reshape(shape), 2, 0)


def direct_lighting(tracer, scene, cam, sampling, params):
    """FF_SHADE_DIFFUSE_PATH_NEE at bounces = 2 in float64 under a camera-sampling setting: nee_ref.direct_lighting's arithmetic,
    vertex for vertex, started from every SAMPLE's own first hit - the twin's ray (ff_camera_sample_rays) through ff_intersect_rays -
    instead of the pixel's G-buffer hit.  Scenes of diffuse surfaces and emitters.  Returns (radiance [H, W, 3], hit mask [H, W]: some
    sample of the pixel hits something, excused mask [H, W]: some shadow or BSDF ray of the pixel may flip between float32 and float64)."""
    assert params.bounces == 2
    W, H, spp = params.width, params.height, params.spp
    key = nee_ref.frame_key(params.seed)
    kinds, le = nee_ref.emission_of(scene)
    albedo = np.array([[b.m_albedo.x, b.m_albedo.y, b.m_albedo.z] for b in (scene.geometries[i].m_bxdf.contents for i in range(len(scene)))], np.float64)
    entries, pdf_area = lib.light_table(scene)
    n_lights = len(entries["area"])
    origins, dirs = frame_rays(cam, sampling, W, H, params.seed, spp)
    out = np.zeros((H, W, 3), np.float64)
    hit_any = np.zeros((H, W), bool)
    excused = np.zeros((H, W), bool)
    for s in range(spp):
        first = tracer.intersect_rays(origins[s].reshape(-1, 3), dirs[s].reshape(-1, 3))
        g_all = np.asarray(first["geom"]).reshape(H, W)
        hit = (np.asarray(first["hit"]).reshape(H, W) != 0) & (g_all >= 0)
        hit_any |= hit
        ys, xs = np.nonzero(hit)
        g0 = g_all[ys, xs]
        emit = kinds[g0] == T.BXDF_EMITTER
        out[ys[emit], xs[emit]] += le[g0[emit]] / spp  # the camera ray's emitter: weight 1
        sel = kinds[g0] == T.BXDF_DIFFUSE
        assert np.all(emit | sel), "diffuse surfaces and emitters only"
        ys, xs, g0 = ys[sel], xs[sel], g0[sel]
        if len(ys) == 0:
            continue
        beta = albedo[g0]
        x = np.asarray(first["point"]).reshape(H, W, 3)[ys, xs].astype(np.float64)
        n = nee_ref._unit(np.asarray(first["normal"]).reshape(H, W, 3)[ys, xs].astype(np.float64))
        d0 = dirs[s][ys, xs].astype(np.float64)
        n = np.where((np.sum(n * d0, -1) > 0.0)[:, None], -n, n)
        gpix = ys.astype(np.uint64) * np.uint64(W) + xs.astype(np.uint64)
        t_basis, s_basis = nee_ref._tangent(n)
        origin = x + nee_ref.RAY_EPS * n
        acc = np.zeros((len(ys), 3), np.float64)
        ctr = np.full(len(ys), (s << 8) | 0, np.uint64)
        # BSDF: cosine-weighted direction about n^ (scatter), then what it hits
        r0, r1 = nee_ref.philox(gpix, ctr, key)
        u1 = nee_ref.u24(r0)
        theta = 2.0 * np.pi * (r1 >> np.uint64(8)).astype(np.float64) / 2.0 ** 24
        rr = np.sqrt(u1)
        lx, ly, lz = rr * np.cos(theta), rr * np.sin(theta), np.sqrt(np.maximum(0.0, 1.0 - u1))
        wo = nee_ref._unit(t_basis * lx[:, None] + s_basis * ly[:, None] + n * lz[:, None])
        hb, flip_b = nee_ref._trace3(tracer, origin, wo, t_basis)
        gb_hit = np.asarray(hb["geom"])
        pb = np.sum(n * wo, -1) / np.pi
        for i in np.nonzero(gb_hit >= 0)[0]:
            g = gb_hit[i]
            if kinds[g] != T.BXDF_EMITTER:
                continue
            w = 1.0
            if pdf_area[g] > 0.0:
                ny = nee_ref._unit(np.array(hb["normal"][i], np.float64))
                cos_y = abs(float(np.dot(ny, wo[i])))
                pl = float(pdf_area[g]) * float(hb["t"][i]) ** 2 / cos_y
                w = pb[i] ** 2 / (pb[i] ** 2 + pl ** 2)
            acc[i] += beta[i] * le[g] * w
        excused[ys[flip_b], xs[flip_b]] = True
        if n_lights > 0:
            # light sample
            a0, a1 = nee_ref.philox(gpix, ctr, key ^ nee_ref.KEY_SELECT)
            q0, q1 = nee_ref.philox(gpix, ctr, key ^ nee_ref.KEY_POINT)
            k = ((a0 * np.uint64(n_lights)) >> np.uint64(32)).astype(np.int64)
            keep = nee_ref.u24(a1) < entries["alias_probability"][k].astype(np.float64)
            k = np.where(keep, k, entries["alias"][k])
            su, sv = nee_ref.u24(q0), nee_ref.u24(q1)
            tri = entries["primitive"][k] >= 0
            r = np.sqrt(su)
            su, sv = np.where(tri, r * (1.0 - sv), su), np.where(tri, r * sv, sv)
            y = entries["v0"][k].astype(np.float64) + su[:, None] * entries["e1"][k] + sv[:, None] * entries["e2"][k]
            dv = y - x
            d2 = np.sum(dv * dv, -1)
            w_dir = dv / np.sqrt(d2)[:, None]
            cos_x = np.sum(n * w_dir, -1)
            cos_y = np.abs(np.sum(entries["normal"][k].astype(np.float64) * w_dir, -1))
            idx = np.nonzero((cos_x > 0.0) & (cos_y > 0.0))[0]
            if len(idx):
                t_sh, _ = nee_ref._tangent(w_dir[idx])
                hs, flip_s = nee_ref._trace3(tracer, origin[idx], w_dir[idx], t_sh)
                g_l = entries["geometry"][k[idx]]
                p_l = entries["primitive"][k[idx]]
                vis = (np.asarray(hs["geom"]) == g_l) & ((p_l < 0) | (np.asarray(hs["tri"]) == p_l))
                pl = pdf_area[g_l].astype(np.float64) * d2[idx] / cos_y[idx]
                pbl = cos_x[idx] / np.pi
                wl = pl ** 2 / (pl ** 2 + pbl ** 2)
                contrib = beta[idx] * le[g_l] * (pbl * wl / pl)[:, None]
                acc[idx[vis]] += contrib[vis]
                excused[ys[idx[flip_s]], xs[idx[flip_s]]] = True
        np.add.at(out, (ys, xs), acc / spp)
    return out, hit_any, excused
