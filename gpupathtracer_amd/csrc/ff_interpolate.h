// ff_interpolate.h — frame generation behind ff_interpolate: the frame of a pose between two rendered frames A and B, made by a
// backward gather.  The in-between pose has its own exact G-buffer (ff_gbuffer is cheap), so every pixel knows its surface point;
// that point is projected through each source's camera, and the colour is fetched there from the 2 x 2 taps that show the same
// surface point.  What neither source shows is filled from same-surface neighbours in a second pass.  The per-pixel functions
// are inline and compiled for the host and the device alike: the kernels (ff_interpolate.hip) and the host twin
// ff_interpolate_host (ff_interpolate_api.cpp) call the same code.  The operator is spelled out in include/firefly/ff_api.h.
//
// Arithmetic: float32 throughout, every expression evaluated as parenthesised below, no fused multiply-add (the library is built
// with -ffp-contract=off), true divisions (correctly rounded on the device under the library's flags).  exp and sqrt appear
// nowhere - distances are compared as squares - so the two sides agree bit for bit.
//
// Not offered: view-dependent re-shading (a mirror's, glass's or glossy highlight's colour is fetched at its surface point, so a
// reflection lags), sources of another size, extrapolation beyond t in [0, 1], a multi-GPU twin.
#pragma once

#include "../../include/firefly/ff_types.h"

#include "ff_pixel.h"
#include "ff_upscale.h" // (UpscaleMean, upscale_clamp: the same mean and the same tap clamp)

namespace ff {

constexpr int kInterpMaxFill = 8; // the largest fill_radius

// A pixel's state after the gather, kept as a float in the work image's w; the fill adds the last two.
constexpr int kInterpBoth = 0, kInterpOnlyA = 1, kInterpOnlyB = 2, kInterpFilled = 3, kInterpFallback = 4;
constexpr float kInterpHole = 3.f; // the gather's mark of a pixel neither source resolved

// One row of the geometry table: the 3 x 4 map of a geometry from the mid pose to a source's pose, and whether it is an identity
// (then x^ = x exactly and nothing is multiplied).  Row 2 g + S belongs to geometry g and source S.
struct InterpMap {
    float4 a[3];
    int identity, pad[3];
};

// One source frame.
struct InterpSource {
    float inv[16];  // inverse(ff_camera_ray_matrix(camera_S)), double on the host, rounded; column-major
    float sw, sh;   // camera_S's m_screenWidth, m_screenHeight
    float eye[3];   // camera_S's m_position
    float pix;      // the world size of a pixel at unit distance: 2 tan(fov / 2) / m_screenHeight, double on the host, rounded
    int cam_rest;   // camera_S is bitwise camera_mid
    const float* radiance;
    const float* position;
    const int* ids;
};

// Everything one call needs; passed by value (kernel arguments).  Images are row-major, top row first.
struct InterpArgs {
    int width, height;
    float t, tol2;          // tol2 = surface_tolerance * surface_tolerance (float)
    int fill_radius;
    int num_geoms;          // rows / 2 of `maps`; 0: no maps (a static scene)
    float ray[16];          // ff_camera_ray_matrix(camera_mid), unjittered: the far point of a miss (kernel.cu:203)
    float inv_mid[16];      // its inverse
    float far_clip, sw, sh; // camera_mid's
    const InterpMap* maps;
    const float* position;  // the mid G-buffer
    const int* ids;
    InterpSource src[2];
};

// Step 1 for source S of pixel (x, y) with geometry index g and surface point xp: where the pixel looks in S's image (hx, hy) and,
// for a hit, its surface point at S's pose xh.  False: the lookup fails.
FF_PIXEL_HD bool interp_lookup(const InterpArgs& a, int S, int x, int y, int g, const float* xp, float& hx, float& hy, float* xh)
{
    const InterpSource& s = a.src[S];
    const bool hit = g >= 0;
    bool identity = true;
    xh[0] = xp[0];
    xh[1] = xp[1];
    xh[2] = xp[2];
    if (hit && a.num_geoms > 0) {
        if (g >= a.num_geoms) return false; // (not known: taa_motion's rule)
        const InterpMap& m = a.maps[2 * g + S];
        identity = m.identity != 0;
        if (!identity) {
            xh[0] = (m.a[0].x * xp[0] + m.a[0].y * xp[1]) + (m.a[0].z * xp[2] + m.a[0].w);
            xh[1] = (m.a[1].x * xp[0] + m.a[1].y * xp[1]) + (m.a[1].z * xp[2] + m.a[1].w);
            xh[2] = (m.a[2].x * xp[0] + m.a[2].y * xp[1]) + (m.a[2].z * xp[2] + m.a[2].w);
        }
    }
    if (s.cam_rest && identity) {
        hx = (float)x; // (nothing is projected)
        hy = (float)y;
        return true;
    }
    float Xx = xh[0], Xy = xh[1], Xz = xh[2], bx = (float)x, by = (float)y;
    if (hit) {
        if (!taa_project(a.inv_mid, xp[0], xp[1], xp[2], a.sw, a.sh, bx, by)) return false; // ~ (x + jx, y + jy)
    } else {
        // kernel.cu:200-203 for the unjittered pixel corner: the far point of the ray (taa_motion's)
        const float Px = ((float)x / a.sw) * 2.f - 1.f, Py = 1.f - ((float)y / a.sh) * 2.f;
        const float v0 = Px * a.far_clip, v1 = Py * a.far_clip, v2 = 1.f * a.far_clip, v3 = 1.f * a.far_clip;
        const float* M = a.ray;
        Xx = (M[0] * v0 + M[4] * v1) + (M[8] * v2 + M[12] * v3);
        Xy = (M[1] * v0 + M[5] * v1) + (M[9] * v2 + M[13] * v3);
        Xz = (M[2] * v0 + M[6] * v1) + (M[10] * v2 + M[14] * v3);
    }
    float fx, fy;
    if (!taa_project(s.inv, Xx, Xy, Xz, s.sw, s.sh, fx, fy)) return false;
    hx = (float)x + (fx - bx);
    hy = (float)y + (fy - by);
    return hx >= 0.f && hy >= 0.f && hx <= (float)(a.width - 1) && hy <= (float)(a.height - 1); // (false for NaN)
}

// Steps 1 and 2 for source S: the colour c_S the pixel finds there.  False: S is not valid for this pixel.
FF_PIXEL_HD bool interp_fetch(const InterpArgs& a, int S, int x, int y, int g, int k, const float* xp, float* c)
{
    const InterpSource& s = a.src[S];
    float hx, hy, xh[3];
    if (!interp_lookup(a, S, x, y, g, xp, hx, hy, xh)) return false;
    const float flx = floorf(hx), fly = floorf(hy);
    const int i0 = (int)flx, j0 = (int)fly;
    const float tx = hx - flx, ty = hy - fly;
    const float bu[2] = { 1.0f - tx, tx }, bv[2] = { 1.0f - ty, ty };
    float limit = 0.f;
    if (g >= 0) {
        const float ex = xh[0] - s.eye[0], ey = xh[1] - s.eye[1], ez = xh[2] - s.eye[2];
        const float D2 = (ex * ex + ey * ey) + ez * ez;
        limit = a.tol2 * (D2 * (s.pix * s.pix));
    }
    UpscaleMean m;
    for (int dj = 0; dj < 2; ++dj) {
        const size_t row = (size_t)upscale_clamp(j0 + dj, a.height - 1) * (size_t)a.width;
        for (int di = 0; di < 2; ++di) {
            const float b = bu[di] * bv[dj];
            if (!(b > 0.f)) continue;
            const size_t q = row + (size_t)upscale_clamp(i0 + di, a.width - 1);
            if (s.ids[3 * q] != g || s.ids[3 * q + 2] != k) continue;
            const float cx = s.radiance[3 * q], cy = s.radiance[3 * q + 1], cz = s.radiance[3 * q + 2];
            if (!(pixel_finite(cx) && pixel_finite(cy) && pixel_finite(cz))) continue;
            if (g >= 0) {
                const float dx = s.position[3 * q] - xh[0], dy = s.position[3 * q + 1] - xh[1], dz = s.position[3 * q + 2] - xh[2];
                const float d2 = (dx * dx + dy * dy) + dz * dz;
                if (!(d2 <= limit)) continue; // (false for NaN)
            }
            m.add(b, cx, cy, cz);
        }
    }
    if (m.n == 0) return false;
    m.get(c);
    return true;
}

// "blend" of ff_api.h for one channel.
FF_PIXEL_HD float interp_blend(float t, float ca, float cb)
{
    if (t == 0.f || ca == cb) return ca;
    if (t == 1.f) return cb;
    return (1.0f - t) * ca + t * cb;
}

// Steps 1 to 3 for pixel (x, y): {rgb, state} of the work image (a hole: rgb 0 and kInterpHole).
FF_PIXEL_HD float4 interp_gather(const InterpArgs& a, int x, int y)
{
    const size_t p = (size_t)y * (size_t)a.width + (size_t)x;
    const int g = a.ids[3 * p], k = a.ids[3 * p + 2];
    const float xp[3] = { a.position[3 * p], a.position[3 * p + 1], a.position[3 * p + 2] };
    float ca[3], cb[3];
    const bool va = interp_fetch(a, 0, x, y, g, k, xp, ca);
    const bool vb = interp_fetch(a, 1, x, y, g, k, xp, cb);
    if (va && vb) return make_float4(interp_blend(a.t, ca[0], cb[0]), interp_blend(a.t, ca[1], cb[1]), interp_blend(a.t, ca[2], cb[2]), (float)kInterpBoth);
    if (va) return make_float4(ca[0], ca[1], ca[2], (float)kInterpOnlyA);
    if (vb) return make_float4(cb[0], cb[1], cb[2], (float)kInterpOnlyB);
    return make_float4(0.f, 0.f, 0.f, kInterpHole);
}

// Step 4's weight of the pixel (dx, dy) away, not both 0.
FF_PIXEL_HD float interp_fill_weight(int dx, int dy) { return 1.0f / (float)(dx * dx + dy * dy); }

// Step 4's last case for pixel p: the screen-space blend of the two sources.
FF_PIXEL_HD void interp_fallback(const InterpArgs& a, size_t p, float* v)
{
    for (int c = 0; c < 3; ++c) v[c] = interp_blend(a.t, a.src[0].radiance[3 * p + c], a.src[1].radiance[3 * p + c]);
}

// The kernels (ff_interpolate.hip): the gather into `work` (W*H float4), then the fill from it into the outputs and the five
// counts (uint32, zeroed by the caller).  rgb8 and radiance_out may be null.
hipError_t launch_interpolate(const InterpArgs& a, float4* work, unsigned char* rgb8, float* radiance_out, uint32_t* counts, hipStream_t stream);

} // namespace ff
