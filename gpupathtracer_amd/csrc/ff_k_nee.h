// ff_k_nee.h — device code of the trace kernels: nee_path_kernel, the next-event-estimation path kernel (a section of ff_kernels.hip).
#pragma once
#include "ff_k_traverse.h"
#include "ff_k_shade.h"

namespace ff {
namespace {

// ---- next-event estimation (FF_SHADE_DIFFUSE_PATH_NEE; the estimator is spelled out in ff_api.h) ------------------------------
//
// One thread per (pixel, sample block) item, persistent: thread t of the launch takes the items t, t + T, t + 2T, ... (T threads;
// item i is pixel item i % pix_items of block i / pix_items, so a wave's lanes start on neighbouring pixels of one tile).  Every
// pass of the loop answers ONE closest-hit query per lane - a path's extension ray or the shadow ray of its last diffuse vertex -
// with the mega-kernels' own closest_hit_deferred / closest_hit_brute, and the path then goes on with the mega-kernels' own scatter().
// A block's samples are summed in order into blocksums[pixel][block] and combine_kernel adds the blocks, so with an empty light table
// every sum is FF_SHADE_DIFFUSE_PATH's bit for bit.  Kept apart from trace_bvh_kernel, which it leaves as it was.
__device__ __forceinline__ float nee_u24(unsigned r) { return (float)(r >> 8) * 5.9604644775390625e-08f; }

// The environment texel direction d falls in (ff_api.h): phi = atan2(d.x, -d.z) - rotation wrapped to [0, 2 pi), theta = acos(d.y),
// nearest texel.  Returns {intensity x rgb, pdf_env}: one 16-byte load.
__device__ __forceinline__ float4 env_lookup(const NeeParams& np, float dx, float dy, float dz)
{
    constexpr float kTwoPi = 6.28318530717958648f, kInvTwoPi = 0.15915494309189535f, kInvPi = 0.31830988618379067f;
    float phi = atan2f(dx, -dz) - np.env_rotation;
    if (phi < 0.f) phi = phi + kTwoPi;
    if (phi < 0.f) phi = phi + kTwoPi;
    const float theta = acosf(fminf(fmaxf(dy, -1.f), 1.f));
    const int c = min(max((int)((phi * kInvTwoPi) * (float)np.env_w), 0), np.env_w - 1);
    const int r = min(max((int)((theta * kInvPi) * (float)np.env_h), 0), np.env_h - 1);
    return np.env_texels[r * np.env_w + c];
}

// ENV = 1: the environment is one more light of the MIS estimator (ff_api.h).  ENV = 0 compiles to the kernel without it.
// TEX = 1: a diffuse hit's albedo is m_albedo times the texel of the texture bound to its geometry (ff_texture.h), looked up at the
// world hit point; FF_SHADE_DIFFUSE_PATH frames of a textured scene run here with no light table, as they do under an environment.
// TEX = 0 compiles to the kernel without it.
// GLOSSY = 1: a mirror whose record has a positive np.glossy_alpha is a GGX conductor (ff_glossy.h; the estimator is in ff_api.h):
// a light sample weighted against the lobe's pdf, then a direction drawn from its visible normals.  The local frame is rebuilt from
// the normal where it is needed; nothing of the lobe stays live across a query but prev_pdf and, for a sample whose direction fell
// below the horizon while its shadow ray is still to be answered, `dead`.  GLOSSY = 0 compiles to the kernel without it.
// CAM = 1: every sample starts with its own camera ray (ff_set_camera_sampling: a point of the pixel, a point of the lens; ff_camera.h)
// in place of the pixel's one primary ray.  A runtime branch in the 32 instantiations without it raised their SGPR spills and, for
// the big-scene ones, their scratch, hence a parameter: CAM = 0 compiles to the kernel without it.

// The first ray of sample P.s.  CAM = 0: the pixel's one primary ray (start_sample).  CAM = 1 (a camera-sampling setting is active):
// the ray camera_sample_ray draws for this sample (ff_camera.h); nothing it computes outlives it but the ray, and the pixel's
// primary direction (P.pdx ..) is neither computed nor kept.
template <int CAM>
__device__ __forceinline__ void nee_start_sample(const NeeParams& np, Path& P)
{
    const KParams& p = np.k;
    if (!CAM) start_sample(p, P);
    else {
        P.b = 0;
        P.bx = P.by = P.bz = 1.f;
        const CameraRays C = { p.cam_c0, p.cam_c1, p.cam_c2, p.cam_c3, p.cam_pos, p.far_clip, p.screen_w, p.screen_h,
                               np.cam_box, np.cam_lens_radius, np.cam_focus, np.cam_fwd, np.cam_right, np.cam_up };
        const unsigned gx = P.gxy & 0xFFFFu, gy = P.gxy >> 16;
        camera_sample_ray(C, (int)gx, (int)gy, gy * (unsigned)p.width + gx, (unsigned)P.s, p.key, P.ray.ox, P.ray.oy, P.ray.oz, P.ray.dx, P.ray.dy,
                          P.ray.dz);
    }
}

// The sample's radiance joins its block's sum and the lane goes on to the next sample or gives its item back (GLOSSY = 1: a sample
// that ends behind its shadow ray; the loop's own ending is the same code).
template <int CAM>
__device__ __forceinline__ bool nee_end_sample(const NeeParams& np, Path& P, float& Lx, float& Ly, float& Lz, float& prev_pdf)
{
    const KParams& p = np.k;
    P.ax = P.ax + Lx;
    P.ay = P.ay + Ly;
    P.az = P.az + Lz;
    Lx = Ly = Lz = 0.f;
    prev_pdf = 0.f;
    ++P.s;
    if (P.s < P.send) {
        nee_start_sample<CAM>(np, P);
        return true;
    }
    p.blocksums[(size_t)((unsigned)P.item & kItemPixelMask) * p.num_blocks + ((unsigned)P.item >> kItemBlockShift)] = make_float4(P.ax, P.ay, P.az, 0.f);
    return false;
}

// The Duff basis about the unit normal u (to_world_about's t and s) and a world direction's components in it.
__device__ __forceinline__ void to_local_about(float ux, float uy, float uz, float wx, float wy, float wz, float& lx, float& ly, float& lz)
{
    const float sign = copysignf(1.0f, uz);
    const float aa = -ieee_rcp(sign + uz);
    const float bb = (ux * uy) * aa;
    const float t0 = 1.0f + ((sign * ux) * ux) * aa, t1 = sign * bb, t2 = -sign * ux;
    const float s0 = bb, s1 = sign + (uy * uy) * aa, s2 = -uy;
    lx = dot3(t0, t1, t2, wx, wy, wz);
    ly = dot3(s0, s1, s2, wx, wy, wz);
    lz = dot3(ux, uy, uz, wx, wy, wz);
}

template <int MODE, int BIG = 0, int ENV = 0, int TEX = 0, int GLOSSY = 0, int CAM = 0>
__global__ __launch_bounds__(kBlockThreads) void nee_path_kernel(const NeeParams np)
{
    const KParams& p = np.k;
    const int tid = threadIdx.x;
    const int lane = tid & (kWave - 1);
    const LdsT<BIG> L = make_lds<BIG>(p.lds_nodes, p.stack_depth, kBlockThreads, tid, p.num_quads, nullptr, p.geoms, p.top_first, p.top_lds_first,
                                      p.top_lds_count, BIG ? p.num_scan : 0, p.stack_spill);
    const uint4* nodes4 = reinterpret_cast<const uint4*>(p.nodes4);
    if (MODE == FF_TRACE_BVH) stage_scene(L, nodes4, p.geoms, p.num_geoms, p.num_planes, tid, kBlockThreads);
    float4* batch = reinterpret_cast<float4*>(ff_smem);
    constexpr float kInvPi = 0.31830988618379067f;
    Counters cnt = {};
    Path P;
    init_path(P);
    unsigned next = blockIdx.x * kBlockThreads + tid;
    const unsigned stride = gridDim.x * kBlockThreads;
    bool active = false;
    float Lx = 0.f, Ly = 0.f, Lz = 0.f; // radiance of the current sample
    float prev_pdf = 0.f;               // pdf_b (solid angle) of the direction the current ray was drawn with; 0: camera or specular
    bool shadow = false;                // the next query is the shadow ray below
    Ray sray = { 0.f, 0.f, 0.f, 0.f, 0.f, 1.f };
    int sgeom = -1, sprim = -1;         // the sampled primitive: record index, caller's triangle index (-1: a plane)
    float scx = 0.f, scy = 0.f, scz = 0.f; // what the light sample adds if the shadow ray reaches it
    bool dead = false;                  // GLOSSY: the sample ends once its pending shadow ray is answered
    for (;;) {
        while (!active && next < np.items) {
            const unsigned item = next;
            next += stride;
            const unsigned blk = item / p.pix_items, pitem = item - blk * p.pix_items;
            const int tile = (int)(pitem >> 6), in = (int)(pitem & 63u);
            const int lx = (tile % p.tiles_per_row) * 8 + (in & 7);
            const int ly = (tile / p.tiles_per_row) * 8 + (in >> 3);
            const int strip = ly / p.strip_rows;
            const int gy = p.y0 + (strip * p.num_parts + p.part) * p.strip_rows + (ly - strip * p.strip_rows);
            const int gx = p.x0 + lx;
            if (lx < p.local_width && gx < p.xlim && ly < p.local_rows && gy < p.ylim) {
                const int block = p.block_begin + (int)blk;
                active = true;
                P.gxy = (unsigned)gx | ((unsigned)gy << 16);
                P.item = (int)(((unsigned)block << kItemBlockShift) | pitem);
                P.s = block * p.block_spp;
                P.send = min(p.spp_total, P.s + p.block_spp);
                P.ax = P.ay = P.az = 0.f;
                if (!CAM) {
                    primary_ray(p, P.gxy, P.ray);
                    P.pdx = P.ray.dx;
                    P.pdy = P.ray.dy;
                    P.pdz = P.ray.dz;
                }
                nee_start_sample<CAM>(np, P);
                Lx = Ly = Lz = 0.f;
                prev_pdf = 0.f;
                shadow = false;
            }
        }
        Best best;
        if (MODE == FF_TRACE_BRUTE_FORCE) {
            if (__syncthreads_or(active ? 1 : 0) == 0) break; // (every thread of the workgroup stages the triangle batches)
            closest_hit_brute<false>(p.geoms, p.num_geoms, p.tris, batch, active, shadow ? sray : P.ray, best, cnt);
        } else {
            if (__ballot(active) == 0ull) break;
            if (active) closest_hit_deferred<false>(L, p.walls, p.geoms, p.num_geoms, p.num_planes, p.tris, nodes4, shadow ? sray : P.ray, best, cnt);
        }
        if (!active) continue;
        if (shadow) {
            // visible iff the closest hit is the sampled primitive itself
            shadow = false;
            if (best.geom == sgeom && (sprim < 0 || (best.rec >= 0 && p.tris[best.rec].orig_index == sprim))) {
                Lx = Lx + scx;
                Ly = Ly + scy;
                Lz = Lz + scz;
            }
            if (GLOSSY && dead) {
                dead = false;
                active = nee_end_sample<CAM>(np, P, Lx, Ly, Lz, prev_pdf);
            }
            continue;
        }
        const bool hit = best.geom >= 0;
        MaterialRef M;
        M.global = p.geoms + (hit ? best.geom : 0);
        M.geom_base = 0;
        M.g = 0;
        bool goes_on = false;
        float galpha = 0.f; // GLOSSY: the lobe width of a glossy hit, 0 at every other hit
        if (hit) {
            const int bxdf = mat_bxdf(M);
            if (GLOSSY && bxdf == FF_BXDF_MIRROR) galpha = np.glossy_alpha[best.geom];
            if (bxdf == FF_BXDF_EMITTER) {
                // BSDF-sampled emitter hit: weight 1 after the camera or a specular bounce and for emitters the table leaves out
                const float4 emission = mat_f4(M, 13);
                float cx = P.bx * emission.x, cy = P.by * emission.y, cz = P.bz * emission.z;
                // (FF_SHADE_DIFFUSE_PATH under an environment runs here with no light table: weight 1)
                const float area_pdf = ((ENV || TEX || GLOSSY || CAM) && np.num_lights == 0) ? 0.f : np.light_pdf[best.geom];
                if (prev_pdf > 0.f && area_pdf > 0.f) {
                    float nx, ny, nz;
                    world_normal(M, best, false, nx, ny, nz);
                    const float ninv = ieee_rcp(ieee_sqrt(dot3(nx, ny, nz, nx, ny, nz)));
                    const float cos_y = fabsf(dot3(nx * ninv, ny * ninv, nz * ninv, P.ray.dx, P.ray.dy, P.ray.dz));
                    float pl = area_pdf * (best.dist * best.dist) / cos_y;
                    if (ENV) pl = pl * np.p_area;
                    const float pb2 = prev_pdf * prev_pdf;
                    const float w = pb2 / (pb2 + pl * pl);
                    cx = cx * w;
                    cy = cy * w;
                    cz = cz * w;
                }
                Lx = Lx + cx;
                Ly = Ly + cy;
                Lz = Lz + cz;
            } else {
                const bool glass = bxdf == FF_BXDF_GLASS;
                float4 albedo = mat_f4(M, 12);
                if (TEX && bxdf == FF_BXDF_DIFFUSE) {
                    float texel[3];
                    if (tex_albedo(np.tex_bind, np.tex_desc, np.uvs, best.geom, best.rec, M.global->type, reinterpret_cast<const float*>(M.global),
                                   reinterpret_cast<const float*>(p.tris), best.px, best.py, best.pz, texel)) {
                        albedo.x = albedo.x * texel[0];
                        albedo.y = albedo.y * texel[1];
                        albedo.z = albedo.z * texel[2];
                    }
                }
                if (!glass && !(GLOSSY && galpha > 0.f)) { // (a glossy hit's throughput takes F G2 / G1 at the scatter)
                    P.bx = P.bx * albedo.x;
                    P.by = P.by * albedo.y;
                    P.bz = P.bz * albedo.z;
                }
                goes_on = P.b != p.bounces - 1;
            }
        } else if (ENV) {
            // BSDF-sampled miss: the environment's radiance, weight 1 after the camera or a specular bounce
            const float4 le = env_lookup(np, P.ray.dx, P.ray.dy, P.ray.dz);
            float cx = P.bx * le.x, cy = P.by * le.y, cz = P.bz * le.z;
            const float pl = np.p_env * le.w;
            if (prev_pdf > 0.f && pl > 0.f) {
                const float pb2 = prev_pdf * prev_pdf;
                const float w = pb2 / (pb2 + pl * pl);
                cx = cx * w;
                cy = cy * w;
                cz = cz * w;
            }
            Lx = Lx + cx;
            Ly = Ly + cy;
            Lz = Lz + cz;
        }
        if (goes_on) {
            const int bxdf = mat_bxdf(M);
            const bool diffuse = bxdf != FF_BXDF_MIRROR && bxdf != FF_BXDF_GLASS;
            const bool glossy = GLOSSY && galpha > 0.f;
            // the flipped unit shading normal scatter() uses
            float ux, uy, uz;
            {
                float nx, ny, nz;
                world_normal(M, best, false, nx, ny, nz);
                const float ninv = ieee_rcp(ieee_sqrt(dot3(nx, ny, nz, nx, ny, nz)));
                ux = nx * ninv; uy = ny * ninv; uz = nz * ninv;
                if (dot3(ux, uy, uz, P.ray.dx, P.ray.dy, P.ray.dz) > 0.0f) { ux = -ux; uy = -uy; uz = -uz; }
            }
            // GLOSSY: wo = minus the ray direction in the local frame (z clamped), F0 = the record's tint (m_specularColor)
            float gox = 0.f, goy = 0.f, goz = 1.f;
            float4 f0 = make_float4(0.f, 0.f, 0.f, 0.f);
            if (glossy) {
                to_local_about(ux, uy, uz, -P.ray.dx, -P.ray.dy, -P.ray.dz, gox, goy, goz);
                goz = fmaxf(goz, kGlossyMinCos);
                f0 = mat_f4(M, 12);
            }
            if ((diffuse || glossy) && (np.num_lights > 0 || (ENV && np.p_env > 0.f))) {
                // light sample: primitive by the alias table, point uniform on it (keys in ff_api.h)
                const unsigned gpix = (P.gxy >> 16) * (unsigned)p.width + (P.gxy & 0xFFFFu);
                const unsigned ctr = ((unsigned)P.s << 8) | ((unsigned)P.b & 0xFFu);
                unsigned r0, r1, q0, q1;
                philox2x32_10(gpix, ctr, p.key ^ kNeeKeySelect, r0, r1);
                philox2x32_10(gpix, ctr, p.key ^ kNeeKeyPoint, q0, q1);
                bool env_pick = false;
                if (ENV) {
                    // the environment or the light table (a stream of its own, drawn only when both are there)
                    env_pick = np.p_env >= 1.f;
                    if (np.p_env > 0.f && np.p_env < 1.f) {
                        unsigned c0, c1;
                        philox2x32_10(gpix, ctr, p.key ^ kEnvKeyChoose, c0, c1);
                        env_pick = nee_u24(c0) < np.p_env;
                    }
                }
                if (ENV && env_pick) {
                    // environment sample: texel by the alias table, direction uniform in solid angle within it
                    int e = (int)(((unsigned long long)r0 * (unsigned long long)(np.env_w * np.env_h)) >> 32);
                    const float2 al = np.env_alias[e];
                    if (!(nee_u24(r1) < al.x)) e = __float_as_int(al.y);
                    const float4 le = np.env_texels[e];
                    const int row = e / np.env_w, col = e - row * np.env_w;
                    const float z0 = np.env_z[row], z1 = np.env_z[row + 1];
                    const float wy = z0 + nee_u24(q0) * (z1 - z0);
                    // phi / pi = (c + v) 2 / W + rotation / pi, in [0, 4): sincospi needs no long argument reduction
                    const float phi_pi = ((float)col + nee_u24(q1)) * (2.0f / (float)np.env_w) + np.env_rotation * kInvPi;
                    const float st = ieee_sqrt(fmaxf(0.f, 1.0f - wy * wy));
                    float sp, cp;
                    sincospif(phi_pi, &sp, &cp);
                    const float wx = st * sp, wz = -(st * cp);
                    const float cos_x = dot3(ux, uy, uz, wx, wy, wz);
                    const float pl = np.p_env * le.w;
                    if (cos_x > 0.f && pl > 0.f) {
                        const float pl2 = pl * pl;
                        if (glossy) {
                            float lx, ly, lz;
                            to_local_about(ux, uy, uz, wx, wy, wz, lx, ly, lz);
                            const GlossyLobe gl = glossy_eval(galpha, f0.x, f0.y, f0.z, gox, goy, goz, lx, ly, cos_x);
                            const float f = (cos_x * (pl2 / (pl2 + gl.pdf * gl.pdf))) / pl; // cos_x * w_l / pdf_l
                            scx = ((P.bx * le.x) * gl.fr) * f;
                            scy = ((P.by * le.y) * gl.fg) * f;
                            scz = ((P.bz * le.z) * gl.fb) * f;
                        } else {
                            const float pb = cos_x * kInvPi;
                            const float f = (pb * (pl2 / (pl2 + pb * pb))) / pl; // (cos_x / pi) * w_l / pdf_l
                            scx = (P.bx * le.x) * f;
                            scy = (P.by * le.y) * f;
                            scz = (P.bz * le.z) * f;
                        }
                        sgeom = -1; // visible iff the shadow ray hits nothing
                        sprim = -1;
                        sray.ox = best.px + ux * kRayEps;
                        sray.oy = best.py + uy * kRayEps;
                        sray.oz = best.pz + uz * kRayEps;
                        sray.dx = wx;
                        sray.dy = wy;
                        sray.dz = wz;
                        shadow = true;
                    }
                } else {
                    int e = (int)(((unsigned long long)r0 * (unsigned long long)np.num_lights) >> 32);
                    const float4 a0 = np.lights[5 * e + 3];
                    if (!(nee_u24(r1) < a0.w)) e = __float_as_int(np.lights[5 * e + 2].w);
                    const float4 v0 = np.lights[5 * e], ea = np.lights[5 * e + 1], eb = np.lights[5 * e + 2], nrm = np.lights[5 * e + 3], ex = np.lights[5 * e + 4];
                    const int prim = __float_as_int(ea.w);
                    float su = nee_u24(q0), sv = nee_u24(q1);
                    if (prim >= 0) { // triangle: the square-root warp
                        const float r = ieee_sqrt(su);
                        su = r * (1.0f - sv);
                        sv = r * sv;
                    }
                    const float yx = v0.x + (su * ea.x + sv * eb.x), yy = v0.y + (su * ea.y + sv * eb.y), yz = v0.z + (su * ea.z + sv * eb.z);
                    const float dx = yx - best.px, dy = yy - best.py, dz = yz - best.pz;
                    const float d2 = dot3(dx, dy, dz, dx, dy, dz);
                    const float dinv = ieee_rcp(ieee_sqrt(d2));
                    const float wx = dx * dinv, wy = dy * dinv, wz = dz * dinv;
                    const float cos_x = dot3(ux, uy, uz, wx, wy, wz);
                    const float cos_y = fabsf(dot3(nrm.x, nrm.y, nrm.z, wx, wy, wz));
                    if (cos_x > 0.f && cos_y > 0.f && d2 > 0.f) {
                        const int g = __float_as_int(v0.w);
                        const float4 le = reinterpret_cast<const float4*>(p.geoms + g)[13];
                        float pl = ex.x * d2 / cos_y;
                        if (ENV) pl = pl * np.p_area;
                        const float pl2 = pl * pl;
                        if (glossy) {
                            float lx, ly, lz;
                            to_local_about(ux, uy, uz, wx, wy, wz, lx, ly, lz);
                            const GlossyLobe gl = glossy_eval(galpha, f0.x, f0.y, f0.z, gox, goy, goz, lx, ly, cos_x);
                            const float f = (cos_x * (pl2 / (pl2 + gl.pdf * gl.pdf))) / pl; // cos_x * w_l / pdf_l
                            scx = ((P.bx * le.x) * gl.fr) * f;
                            scy = ((P.by * le.y) * gl.fg) * f;
                            scz = ((P.bz * le.z) * gl.fb) * f;
                        } else {
                            const float pb = cos_x * kInvPi;
                            const float f = (pb * (pl2 / (pl2 + pb * pb))) / pl; // (cos_x / pi) * w_l / pdf_l
                            scx = (P.bx * le.x) * f;
                            scy = (P.by * le.y) * f;
                            scz = (P.bz * le.z) * f;
                        }
                        sgeom = g;
                        sprim = prim;
                        sray.ox = best.px + ux * kRayEps;
                        sray.oy = best.py + uy * kRayEps;
                        sray.oz = best.pz + uz * kRayEps;
                        sray.dx = wx;
                        sray.dy = wy;
                        sray.dz = wz;
                        shadow = true;
                    }
                }
            }
            if (glossy) {
                // the numbers the diffuse scatter would have drawn at this vertex; the direction from the lobe's visible normals
                const unsigned gpix = (P.gxy >> 16) * (unsigned)p.width + (P.gxy & 0xFFFFu);
                unsigned r0, r1;
                philox2x32_10(gpix, ((unsigned)P.s << 8) | ((unsigned)P.b & 0xFFu), p.key, r0, r1);
                float lx, ly, lz;
                const GlossyLobe gl = glossy_sample(galpha, f0.x, f0.y, f0.z, gox, goy, goz, r0 >> 8, nee_u24(r1), lx, ly, lz);
                if (lz > 0.f) {
                    P.bx = P.bx * gl.wr;
                    P.by = P.by * gl.wg;
                    P.bz = P.bz * gl.wb;
                    float wox, woy, woz;
                    to_world_about(ux, uy, uz, lx, ly, lz, wox, woy, woz);
                    P.ray.ox = best.px + ux * kRayEps;
                    P.ray.oy = best.py + uy * kRayEps;
                    P.ray.oz = best.pz + uz * kRayEps;
                    P.ray.dx = wox;
                    P.ray.dy = woy;
                    P.ray.dz = woz;
                    ++P.b;
                    prev_pdf = gl.pdf;
                    continue;
                }
                // below the horizon: the sample ends at this vertex, behind its shadow ray if one is pending
                if (shadow) {
                    dead = true;
                    continue;
                }
            } else {
                scatter<true>(p, best, M, P);
                prev_pdf = diffuse ? dot3(ux, uy, uz, P.ray.dx, P.ray.dy, P.ray.dz) * kInvPi : 0.f;
                continue;
            }
        }
        // the sample ends here: its radiance joins the block's sum
        P.ax = P.ax + Lx;
        P.ay = P.ay + Ly;
        P.az = P.az + Lz;
        Lx = Ly = Lz = 0.f;
        prev_pdf = 0.f;
        ++P.s;
        if (P.s < P.send) {
            nee_start_sample<CAM>(np, P);
        } else {
            p.blocksums[(size_t)((unsigned)P.item & kItemPixelMask) * p.num_blocks + ((unsigned)P.item >> kItemBlockShift)] = make_float4(P.ax, P.ay, P.az, 0.f);
            active = false;
        }
    }
    flush_counters(p, lane, cnt, false);
}

} // namespace
} // namespace ff
