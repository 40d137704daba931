// ff_camera.h — the per-sample camera ray (ff_set_camera_sampling): a box pixel filter and a thin lens, as inline functions compiled
// for the host and the device alike.  nee_path_kernel (ff_k_nee.h) draws every sample's first ray with camera_sample_ray while a
// setting is active, and the host twin ff_camera_sample_rays (ff_camera.cpp) calls the same function, so the integrator and the host
// agree on every operation.  The estimator is spelled out in ff_api.h.
//
// Arithmetic: float32 throughout, every expression evaluated exactly as parenthesised below, no fused multiply-add (the library is
// built with -ffp-contract=off).  Quotients by a computed length are a * rcp(b) and roots sqrt(x), both correctly rounded:
// FF_CAMERA_RCP / FF_CAMERA_SQRT are the kernels' ieee_rcp / ieee_sqrt on the device (ff_k_core.h defines them before it includes
// this file) and 1.0f / x, sqrtf on the host - the same bits.  The lens point's sine and cosine are ff_glossy.h's fixed-order
// polynomials on an exactly reduced octant.  The random numbers are Philox2x32-10 outputs: integers, the same everywhere.
//
//   pinhole   Px = (((float)x + fx) / screen_w) * 2 - 1,  Py = 1 - (((float)y + fy) / screen_h) * 2;  the rest is primary_ray's
//             arithmetic operation for operation (fx = fy = 0: primary_ray's ray bit for bit)
//   box       (a0, a1) = Philox(gpix, s << 8, key ^ kCameraKeyPixel);  fx = u24(a0), fy = u24(a1)
//   lens      c = dot(d, f^);  !(c > 1e-6): the pinhole ray.  Else t = focus * rcp(c), F = o + d t;
//             (l0, l1) = Philox(gpix, s << 8, key ^ kCameraKeyLens);  (sn, cs) = glossy_sincos_turn(l0 >> 8);
//             rho = radius * sqrt(u24(l1)), a = rho cs, b = rho sn;  o' = o + (a r^ + b u^);  d' = (F - o') * rcp(|F - o'|)
#pragma once

#include <math.h>

#include "ff_glossy.h"
#include "ff_kernels.h"

#if defined(FF_CAMERA_HD)
// (ff_k_core.h: device only, with the kernels' own reciprocal and root)
#elif defined(__HIPCC__)
#define FF_CAMERA_HD __host__ __device__ __forceinline__
#else
#define FF_CAMERA_HD inline
#endif

#ifndef FF_CAMERA_RCP
#define FF_CAMERA_RCP(x) (1.0f / (x))
#define FF_CAMERA_SQRT(x) sqrtf(x)
#endif

namespace ff {

constexpr float kCameraMinCos = 1.0e-6f; // a pinhole direction at or below this cosine to m_forward keeps the pinhole ray

// The frame's camera as the kernels hold it (KParams::cam_*, NeeParams::cam_*): the ray matrix's columns, the position, the far
// plane, the screen size as floats; then the setting: box != 0 draws the pixel point, lens_radius > 0 the lens point.
struct CameraRays {
    const float *c0, *c1, *c2, *c3; // 4 floats each
    const float* pos;               // 3 floats
    float far_clip, screen_w, screen_h;
    int box;
    float lens_radius, focus;
    const float *fwd, *right, *up;  // m_forward, m_right, m_up as the caller's floats (read only when lens_radius > 0)
};

// Philox2x32-10 (ff_k_shade.h philox2x32_10, the same integers)
FF_CAMERA_HD void camera_philox(unsigned c0, unsigned c1, unsigned key, unsigned& o0, unsigned& o1)
{
    for (int r = 0; r < 10; ++r) {
        if (r > 0) key += 0x9E3779B9u;
        const unsigned long long prod = (unsigned long long)c0 * 0xD256D193ull;
        c0 = (unsigned)(prod >> 32) ^ key ^ c1;
        c1 = (unsigned)prod;
    }
    o0 = c0;
    o1 = c1;
}

FF_CAMERA_HD float camera_u24(unsigned r) { return (float)(r >> 8) * 5.9604644775390625e-08f; }

FF_CAMERA_HD float camera_dot3(float ax, float ay, float az, float bx, float by, float bz)
{
    const float px = ax * bx, py = ay * by, pz = az * bz;
    return (px + py) + pz;
}

// primary_ray (ff_k_shade.h) through the point (x + fx, y + fy) of the pixel grid: the unit direction from the camera position.
FF_CAMERA_HD void camera_pinhole(const CameraRays& C, int x, int y, float fx, float fy, float& dx, float& dy, float& dz)
{
    const float Px = (((float)x + fx) / C.screen_w) * 2.f - 1.f;
    const float Py = 1.f - (((float)y + fy) / C.screen_h) * 2.f;
    const float v0 = Px * C.far_clip, v1 = Py * C.far_clip, v2 = 1.f * C.far_clip, v3 = 1.f * C.far_clip;
    const float wx = (C.c0[0] * v0 + C.c1[0] * v1) + (C.c2[0] * v2 + C.c3[0] * v3);
    const float wy = (C.c0[1] * v0 + C.c1[1] * v1) + (C.c2[1] * v2 + C.c3[1] * v3);
    const float wz = (C.c0[2] * v0 + C.c1[2] * v1) + (C.c2[2] * v2 + C.c3[2] * v3);
    const float ddx = wx - C.pos[0], ddy = wy - C.pos[1], ddz = wz - C.pos[2];
    const float inv = FF_CAMERA_RCP(FF_CAMERA_SQRT(camera_dot3(ddx, ddy, ddz, ddx, ddy, ddz)));
    dx = ddx * inv;
    dy = ddy * inv;
    dz = ddz * inv;
}

// The ray of sample s of global pixel (x, y), gpix = y * width + x, under the frame key: origin o[3], unit direction d[3].
FF_CAMERA_HD void camera_sample_ray(const CameraRays& C, int x, int y, unsigned gpix, unsigned s, unsigned key, float& ox, float& oy, float& oz,
                                    float& dx, float& dy, float& dz)
{
    float fx = 0.f, fy = 0.f;
    if (C.box) {
        unsigned a0, a1;
        camera_philox(gpix, s << 8, key ^ kCameraKeyPixel, a0, a1);
        fx = camera_u24(a0);
        fy = camera_u24(a1);
    }
    camera_pinhole(C, x, y, fx, fy, dx, dy, dz);
    ox = C.pos[0];
    oy = C.pos[1];
    oz = C.pos[2];
    if (!(C.lens_radius > 0.f)) return;
    const float c = camera_dot3(dx, dy, dz, C.fwd[0], C.fwd[1], C.fwd[2]);
    if (!(c > kCameraMinCos)) return;
    const float t = C.focus * FF_CAMERA_RCP(c);
    const float Fx = ox + dx * t, Fy = oy + dy * t, Fz = oz + dz * t; // the pinhole ray's point in the plane of focus
    unsigned l0, l1;
    camera_philox(gpix, s << 8, key ^ kCameraKeyLens, l0, l1);
    float sn, cs;
    glossy_sincos_turn(l0 >> 8, sn, cs);
    const float rho = C.lens_radius * FF_CAMERA_SQRT(camera_u24(l1));
    const float a = rho * cs, b = rho * sn;
    ox = ox + (a * C.right[0] + b * C.up[0]);
    oy = oy + (a * C.right[1] + b * C.up[1]);
    oz = oz + (a * C.right[2] + b * C.up[2]);
    const float ex = Fx - ox, ey = Fy - oy, ez = Fz - oz;
    const float inv = FF_CAMERA_RCP(FF_CAMERA_SQRT(camera_dot3(ex, ey, ez, ex, ey, ez)));
    dx = ex * inv;
    dy = ey * inv;
    dz = ez * inv;
}

} // namespace ff
