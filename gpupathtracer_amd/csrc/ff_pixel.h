// ff_pixel.h — the per-pixel helpers the image filters share (ff_motion_blur.h, ff_dof.h, ff_upscale.h, ff_taa_common.h), compiled
// for the host and the device alike: the finiteness test, the clamp to 0 .. 1, the 8-bit rule, the hash of a pixel's place and the
// store of a result pixel.  The trace kernels keep their own (ff_k_shade.h to_u8) and include nothing from here.  Every expression
// is evaluated as parenthesised (the library is built with -ffp-contract=off): the filters' host twins agree with the kernels bit
// for bit through these bodies.
#pragma once

#include <float.h>
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include <hip/hip_runtime.h>

#if defined(__HIPCC__)
#define FF_PIXEL_HD __host__ __device__ __forceinline__
#else
#define FF_PIXEL_HD inline
#endif

namespace ff {

FF_PIXEL_HD bool pixel_finite(float v) { return fabsf(v) <= FLT_MAX; } // (false for NaN)

FF_PIXEL_HD float pixel_clamp01(float v) { return v < 0.f ? 0.f : (v > 1.f ? 1.f : v); }

FF_PIXEL_HD unsigned char pixel_u8(float v)
{
    // the project's 8-bit rule (kernel.cu:214 truncation, out-of-range values clamped, NaN -> 0): ff_k_shade.h to_u8
    const float s = v * 255.0f;
    if (!(s > 0.0f)) return 0;
    if (s >= 255.0f) return 255;
    return (unsigned char)s;
}

// The hash of pixel (x, y) behind the filters' per-pixel jitter.
FF_PIXEL_HD uint32_t pixel_hash(int x, int y)
{
    uint32_t h = ((uint32_t)x * 0x9E3779B1u) ^ ((uint32_t)y * 0x85EBCA77u);
    h ^= h >> 15;
    h *= 0x2C1B3C6Du;
    h ^= h >> 12;
    return h;
}

FF_PIXEL_HD float pixel_u24(uint32_t h) { return (float)(h >> 8) * 5.9604644775390625e-08f - 0.5f; } // 2^-24; [-0.5, 0.5)

// P(M, X) of ff_api.h (ff_taa, ff_taa_upscale, ff_interpolate): q = inverse(M) (X, 1), P the inverse, column-major; false when
// q.w <= 0 (or NaN)
FF_PIXEL_HD bool taa_project(const float* P, float x, float y, float z, float sw, float sh, float& fx, float& fy)
{
    const float qx = (P[0] * x + P[4] * y) + (P[8] * z + P[12]);
    const float qy = (P[1] * x + P[5] * y) + (P[9] * z + P[13]);
    const float qw = (P[3] * x + P[7] * y) + (P[11] * z + P[15]);
    if (!(qw > 0.f)) return false;
    fx = (qx / qw + 1.f) * 0.5f * sw;
    fy = (1.f - qy / qw) * 0.5f * sh;
    return true;
}

// Pixel i's result v[3] into the outputs that are there.
FF_PIXEL_HD void store_rgb(size_t i, const float* v, unsigned char* rgb8, float* radiance_out)
{
    if (radiance_out) { radiance_out[3 * i] = v[0]; radiance_out[3 * i + 1] = v[1]; radiance_out[3 * i + 2] = v[2]; }
    if (rgb8) { rgb8[3 * i] = pixel_u8(v[0]); rgb8[3 * i + 1] = pixel_u8(v[1]); rgb8[3 * i + 2] = pixel_u8(v[2]); }
}

} // namespace ff
