// ff_upscale.h — G-buffer-guided upsampling behind ff_upscale (Kopf et al. 2007's joint bilateral upsampling with the edge-stopping
// functions of ff_denoise): a w x h radiance image and its G-buffer, plus the W x H G-buffer of the same view, give a W x H image.
// The per-pixel function is inline and compiled for the host and the device alike: the kernel (ff_upscale.hip) and the host twin
// ff_upscale_host (ff_upscale_api.cpp) call the same code.  The operator is spelled out in include/firefly/ff_api.h.
//
// Arithmetic: float32 throughout, every expression evaluated as parenthesised below, no fused multiply-add (the library is built
// with -ffp-contract=off), true divisions and square roots (correctly rounded on the device under the library's flags, so the two
// sides differ only in expf).  A dot product is (x + y) + z, as everywhere in the library.
//
// Not offered: upscaling ff_denoise_temporal's history, non-uniform or foveated sampling, a multi-GPU twin.  (The temporal
// upsampler is ff_taa_upscale: ff_taa_upscale.h.)
#pragma once

#include <math.h>
#include <stddef.h>

#include <hip/hip_runtime.h>

#include "../../include/firefly/ff_types.h"
#include "ff_pixel.h"

#if defined(__HIPCC__)
#define FF_UPSCALE_HD __host__ __device__ __forceinline__
#else
#define FF_UPSCALE_HD inline
#endif

namespace ff {

constexpr float kUpscalePlaneEps = 1e-30f;   // keeps |x_q - x_P|^2 = 0 finite (ff_denoise's)
constexpr float kUpscaleMaxExponent = 30.f;  // a tap whose w_n w_x is below e^-30 weighs 0 (ff_denoise's cut-off)

// Everything one call needs; passed by value (kernel arguments).  Images are row-major, top row first, three values per pixel.
struct UpscaleArgs {
    int lo_width, lo_height, width, height;
    float sigma_normal, sigma_plane2; // sigma_plane2 = sigma_plane * sigma_plane (float)
    float lo_jx, lo_jy, hi_jx, hi_jy;
    int same_geometry, demodulate;
    const float *radiance_lo, *position_lo, *normal_lo, *albedo_lo; // albedo_lo, albedo: read only when demodulate != 0
    const int* ids_lo;
    const float *position, *normal, *albedo;
    const int* ids;
};

FF_UPSCALE_HD float upscale_dot3(float ax, float ay, float az, float bx, float by, float bz)
{
    const float px = ax * bx, py = ay * by, pz = az * bz;
    return (px + py) + pz;
}

FF_UPSCALE_HD bool upscale_filterable(int geom, int bxdf)
{
    return geom >= 0 && bxdf != FF_BXDF_EMITTER && bxdf != FF_BXDF_MIRROR && bxdf != FF_BXDF_GLASS;
}

FF_UPSCALE_HD int upscale_clamp(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// The weighted mean of the taps that count, as c_0 + sum w (c_q - c_0) / sum w with c_0 the first of them: equal to
// sum w c_q / sum w, and a single tap, or a colour every tap shares, comes back bit for bit.
struct UpscaleMean {
    int n = 0;
    float wsum = 0.f;
    float c0[3] = { 0.f, 0.f, 0.f }, s[3] = { 0.f, 0.f, 0.f };
    FF_UPSCALE_HD void add(float w, float cx, float cy, float cz)
    {
        if (n == 0) {
            c0[0] = cx;
            c0[1] = cy;
            c0[2] = cz;
        } else {
            s[0] += w * (cx - c0[0]);
            s[1] += w * (cy - c0[1]);
            s[2] += w * (cz - c0[2]);
        }
        wsum += w;
        ++n;
    }
    FF_UPSCALE_HD void get(float* out) const
    {
        for (int k = 0; k < 3; ++k) out[k] = n == 1 ? c0[k] : c0[k] + s[k] / wsum;
    }
};

// The taps of step 1 in the order they are named, row by row: first the 2x2 taps whose bilinear weight b is > 0; if tap(q, b) took
// none of them (it returns whether the tap counted), the 4x4 taps with b = 1.  q: the clamped tap's pixel index in the low image.
// Returns whether any tap counted.
template <class Tap>
FF_UPSCALE_HD bool upscale_taps(const UpscaleArgs& a, int i0, int j0, float fu, float fv, Tap tap)
{
    const int w = a.lo_width, h = a.lo_height;
    const float bu[2] = { 1.0f - fu, fu }, bv[2] = { 1.0f - fv, fv };
    bool any = false;
    for (int round = 0; round < 2 && !any; ++round) {
        const int first = round == 0 ? 0 : -1, last = round == 0 ? 1 : 2;
        for (int dj = first; dj <= last; ++dj) {
            const size_t row = (size_t)upscale_clamp(j0 + dj, h - 1) * (size_t)w;
            for (int di = first; di <= last; ++di) {
                float b = 1.0f;
                if (round == 0) {
                    b = bu[di] * bv[dj];
                    if (!(b > 0.f)) continue;
                }
                if (tap(row + (size_t)upscale_clamp(i0 + di, w - 1), b)) any = true;
            }
        }
    }
    return any;
}

// High pixel (X, Y) of ff_upscale (ff_api.h steps 1-4) into out[3].
FF_UPSCALE_HD void upscale_pixel(const UpscaleArgs& a, int X, int Y, float* out)
{
    const int w = a.lo_width, h = a.lo_height;
    const size_t P = (size_t)Y * (size_t)a.width + (size_t)X;
    // 1. where the pixel looks in the low image
    const float u = (((float)X + a.hi_jx) * (float)w) / (float)a.width - a.lo_jx;
    const float v = (((float)Y + a.hi_jy) * (float)h) / (float)a.height - a.lo_jy;
    const float flu = floorf(u), flv = floorf(v);
    const int i0 = (int)flu, j0 = (int)flv;
    const float fu = u - flu, fv = v - flv;
    const int gP = a.ids[3 * P], kP = a.ids[3 * P + 2];
    UpscaleMean m;
    if (upscale_filterable(gP, kP)) {
        // 2. the pixel's guides; the taps weigh b w_n w_x
        const float xP = a.position[3 * P], yP = a.position[3 * P + 1], zP = a.position[3 * P + 2];
        float nx = a.normal[3 * P], ny = a.normal[3 * P + 1], nz = a.normal[3 * P + 2];
        const float n2 = upscale_dot3(nx, ny, nz, nx, ny, nz);
        const float inv = n2 > 0.f ? 1.0f / sqrtf(n2) : 0.f; // (the G-buffer normal is not unit length under non-uniform scale)
        nx *= inv;
        ny *= inv;
        nz *= inv;
        float aP[3] = { 0.f, 0.f, 0.f };
        if (a.demodulate) {
            aP[0] = a.albedo[3 * P];
            aP[1] = a.albedo[3 * P + 1];
            aP[2] = a.albedo[3 * P + 2];
        }
        const bool any = upscale_taps(a, i0, j0, fu, fv, [&](size_t q, float b) {
            const int gq = a.ids_lo[3 * q];
            if (!upscale_filterable(gq, a.ids_lo[3 * q + 2]) || (a.same_geometry && gq != gP)) return false;
            float c[3] = { a.radiance_lo[3 * q], a.radiance_lo[3 * q + 1], a.radiance_lo[3 * q + 2] };
            if (!(pixel_finite(c[0]) && pixel_finite(c[1]) && pixel_finite(c[2]))) return false;
            if (a.demodulate) {
                const float aq[3] = { a.albedo_lo[3 * q], a.albedo_lo[3 * q + 1], a.albedo_lo[3 * q + 2] };
                if ((aP[0] > 0.f && !(aq[0] > 0.f)) || (aP[1] > 0.f && !(aq[1] > 0.f)) || (aP[2] > 0.f && !(aq[2] > 0.f))) return false;
                for (int k = 0; k < 3; ++k)
                    if (aP[k] > 0.f) c[k] = c[k] / aq[k];
            }
            float qx = a.normal_lo[3 * q], qy = a.normal_lo[3 * q + 1], qz = a.normal_lo[3 * q + 2];
            const float q2 = upscale_dot3(qx, qy, qz, qx, qy, qz);
            const float qinv = q2 > 0.f ? 1.0f / sqrtf(q2) : 0.f;
            qx *= qinv;
            qy *= qinv;
            qz *= qinv;
            const float a_n = (1.0f - upscale_dot3(nx, ny, nz, qx, qy, qz)) / a.sigma_normal;
            const float vx = a.position_lo[3 * q] - xP, vy = a.position_lo[3 * q + 1] - yP, vz = a.position_lo[3 * q + 2] - zP;
            const float pd = upscale_dot3(nx, ny, nz, vx, vy, vz);
            const float a_x = (pd * pd) / (a.sigma_plane2 * upscale_dot3(vx, vy, vz, vx, vy, vz) + kUpscalePlaneEps);
            const float e = a_n + a_x;
            if (!(e <= kUpscaleMaxExponent)) return false;
            m.add(b * expf(-e), c[0], c[1], c[2]);
            return true;
        });
        if (any) {
            m.get(out);
            for (int k = 0; k < 3; ++k)
                if (aP[k] > 0.f) out[k] = out[k] * aP[k]; // (aP is 0 without demodulation)
            return;
        }
    } else {
        // 3. a miss, an emitter, a mirror or glass: the taps of the same geometry and kind weigh b
        const bool any = upscale_taps(a, i0, j0, fu, fv, [&](size_t q, float b) {
            if (a.ids_lo[3 * q] != gP || a.ids_lo[3 * q + 2] != kP) return false;
            const float cx = a.radiance_lo[3 * q], cy = a.radiance_lo[3 * q + 1], cz = a.radiance_lo[3 * q + 2];
            if (!(pixel_finite(cx) && pixel_finite(cy) && pixel_finite(cz))) return false;
            m.add(b, cx, cy, cz);
            return true;
        });
        if (any) {
            m.get(out);
            return;
        }
    }
    // 4. nothing to interpolate from: the nearest low pixel as it is
    const size_t q = (size_t)upscale_clamp((int)floorf(v + 0.5f), h - 1) * (size_t)w + (size_t)upscale_clamp((int)floorf(u + 0.5f), w - 1);
    out[0] = a.radiance_lo[3 * q];
    out[1] = a.radiance_lo[3 * q + 1];
    out[2] = a.radiance_lo[3 * q + 2];
}

// One launch: 64 x 4 pixels per workgroup, a wave on 64 consecutive pixels of a row.  rgb8 and radiance_out may be null.
hipError_t launch_upscale(const UpscaleArgs& a, unsigned char* rgb8, float* radiance_out, hipStream_t stream);

} // namespace ff
