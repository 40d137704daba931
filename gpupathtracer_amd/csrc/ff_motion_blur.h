// ff_motion_blur.h — the motion-blur reconstruction filter behind ff_motion_blur (McGuire, Hennessy, Bukowski and Osman, "A
// Reconstruction Filter for Plausible Motion Blur", I3D 2012, without the diagonal-tile rule): a W x H radiance image, the per-pixel
// screen motion the *_history calls hand out and ff_gbuffer's depth give a W x H image blurred along the motion.  The per-pixel
// functions of steps 1, 3 and 4 are inline and compiled for the host and the device alike: the kernels (ff_motion_blur.hip) and the
// host twin ff_motion_blur_host (ff_motion_blur_api.cpp) call the same code.  The operator is spelled out in include/firefly/ff_api.h.
//
// Arithmetic: float32 throughout, every expression evaluated as parenthesised below, no fused multiply-add (the library is built
// with -ffp-contract=off), true divisions and square roots (correctly rounded on the device under the library's flags).  exp and pow
// appear nowhere, so the two sides agree bit for bit.
//
// Not offered: time-sampled blur in the path kernels, motion of deforming meshes, the diagonal-tile rule, per-tile sample counts,
// a multi-GPU twin.
#pragma once

#include <float.h>
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <hip/hip_runtime.h>

#include "../../include/firefly/ff_types.h"

#if defined(__HIPCC__)
#define FF_MBLUR_HD __host__ __device__ __forceinline__
#else
#define FF_MBLUR_HD inline
#endif

namespace ff {

// Everything one call needs besides its buffers; passed by value (kernel arguments).  Images are row-major, top row first.
struct MotionBlurArgs {
    int width, height;
    int k;              // max_radius: the longest half-spread and the tile edge
    int samples;        // S
    int tiles_x, tiles_y; // ceil(width / k), ceil(height / k)
    float half_shutter; // 0.5f * shutter, formed once
    float depth_extent;
};

FF_MBLUR_HD bool mblur_finite(float v) { return fabsf(v) <= 3.402823466e+38f; } // (false for NaN)

FF_MBLUR_HD float mblur_clamp01(float v) { return v < 0.f ? 0.f : (v > 1.f ? 1.f : v); }

FF_MBLUR_HD uint32_t mblur_bits(float v)
{
    uint32_t b;
    memcpy(&b, &v, sizeof b);
    return b;
}

FF_MBLUR_HD unsigned char mblur_u8(float v)
{
    // the project's 8-bit rule (truncation, out-of-range values clamped): ff_k_shade.h to_u8
    const float s = v * 255.0f;
    if (!(s > 0.0f)) return 0;
    if (s >= 255.0f) return 255;
    return (unsigned char)s;
}

// Step 1 for one pixel: {v.x, v.y, l, z} from its motion m and its depth.
FF_MBLUR_HD float4 mblur_pack(const MotionBlurArgs& a, float mx, float my, float depth)
{
    float vx = mx * a.half_shutter, vy = my * a.half_shutter;
    if (!(mblur_finite(vx) && mblur_finite(vy))) vx = vy = 0.f;
    float l = sqrtf(vx * vx + vy * vy);
    if (l > (float)a.k) {
        const float s = (float)a.k / l;
        vx = vx * s;
        vy = vy * s;
        l = sqrtf(vx * vx + vy * vy);
    }
    const float z = (mblur_finite(depth) && depth > 0.f) ? depth : FLT_MAX;
    return make_float4(vx, vy, l, z);
}

// The key of steps 2 and 3: the float bits of the squared length above an inverted index, so that the largest key is the largest
// squared length and, among equals, the smallest index.  (The squared length is >= +0 and finite or +Inf: its bits are ordered.)
FF_MBLUR_HD unsigned long long mblur_key(float vx, float vy, unsigned index)
{
    return ((unsigned long long)mblur_bits(vx * vx + vy * vy) << 32) | (unsigned long long)(0xFFFFFFFFu - index);
}

// Step 3 for tile (tx, ty): the largest T over the 3x3 tiles around it that exist, ties to the first in row-major order.
FF_MBLUR_HD float4 mblur_neighbour_max(const MotionBlurArgs& a, const float4* tile_max, int tx, int ty)
{
    unsigned long long best = 0;
    float4 out = make_float4(0.f, 0.f, 0.f, 0.f);
    unsigned n = 0;
    for (int dy = -1; dy <= 1; ++dy)
        for (int dx = -1; dx <= 1; ++dx, ++n) {
            const int qx = tx + dx, qy = ty + dy;
            if (qx < 0 || qy < 0 || qx >= a.tiles_x || qy >= a.tiles_y) continue;
            const float4 t = tile_max[(size_t)qy * (size_t)a.tiles_x + (size_t)qx];
            const unsigned long long key = mblur_key(t.x, t.y, n);
            if (key > best) {
                best = key;
                out = t;
            }
        }
    return out;
}

FF_MBLUR_HD float mblur_soft(float za, float zb, float extent) { return mblur_clamp01(1.f - (za - zb) / extent); }

FF_MBLUR_HD float mblur_cone(float d, float l) { return l > 0.f ? mblur_clamp01(1.f - d / l) : 0.f; }

FF_MBLUR_HD float mblur_cylinder(float d, float l)
{
    if (!(l > 0.f)) return 0.f;
    const float lo = 0.95f * l, hi = 1.05f * l;
    const float u = mblur_clamp01((d - lo) / (hi - lo));
    return 1.f - ((u * u) * (3.f - (2.f * u)));
}

// Step 4's jitter for pixel (x, y): j in [-0.5, 0.5).
FF_MBLUR_HD float mblur_jitter(int x, int y)
{
    uint32_t h = ((uint32_t)x * 0x9E3779B1u) ^ ((uint32_t)y * 0x85EBCA77u);
    h ^= h >> 15;
    h *= 0x2C1B3C6Du;
    h ^= h >> 12;
    return (float)(h >> 8) * 5.9604644775390625e-08f - 0.5f; // 2^-24
}

// Step 4 for pixel (x, y) into out[3].  plane: step 1's {v, l, z} per pixel; n: N of the pixel's tile.
FF_MBLUR_HD void mblur_gather(const MotionBlurArgs& a, int x, int y, const float4* plane, const float* radiance, float4 n, float* out)
{
    const size_t X = (size_t)y * (size_t)a.width + (size_t)x;
    const float cX[3] = { radiance[3 * X], radiance[3 * X + 1], radiance[3 * X + 2] };
    out[0] = cX[0];
    out[1] = cX[1];
    out[2] = cX[2];
    if (n.z <= 0.5f || !(mblur_finite(cX[0]) && mblur_finite(cX[1]) && mblur_finite(cX[2]))) return;
    const float4 pX = plane[X];
    const float lX = pX.z, zX = pX.w;
    const float j = mblur_jitter(x, y);
    const float steps = (float)(a.samples + 1);
    float asum = 0.f, s[3] = { 0.f, 0.f, 0.f };
    for (int i = 0; i < a.samples; ++i) {
        const float t = ((((float)i + j) + 1.f) / steps) * 2.f - 1.f;
        const int dx = (int)floorf(n.x * t + 0.5f), dy = (int)floorf(n.y * t + 0.5f);
        const int qx = x + dx, qy = y + dy;
        if ((dx == 0 && dy == 0) || qx < 0 || qy < 0 || qx >= a.width || qy >= a.height) continue;
        const size_t Y = (size_t)qy * (size_t)a.width + (size_t)qx;
        const float cY[3] = { radiance[3 * Y], radiance[3 * Y + 1], radiance[3 * Y + 2] };
        if (!(mblur_finite(cY[0]) && mblur_finite(cY[1]) && mblur_finite(cY[2]))) continue;
        const float4 pY = plane[Y];
        const float lY = pY.z, zY = pY.w;
        const float d = sqrtf((float)(dx * dx + dy * dy));
        const float f = mblur_soft(zY, zX, a.depth_extent), b = mblur_soft(zX, zY, a.depth_extent);
        const float w = (f * mblur_cone(d, lY) + b * mblur_cone(d, lX)) + (mblur_cylinder(d, lY) * mblur_cylinder(d, lX)) * 2.f;
        s[0] = s[0] + w * (cY[0] - cX[0]);
        s[1] = s[1] + w * (cY[1] - cX[1]);
        s[2] = s[2] + w * (cY[2] - cX[2]);
        asum = asum + w;
    }
    const float w0 = 1.f / (lX > 0.5f ? lX : 0.5f);
    const float wsum = w0 + asum;
    // (a channel whose sum is 0 keeps the centre's bits: cX + 0 would turn -0 into +0)
    for (int c = 0; c < 3; ++c)
        if (s[c] != 0.f) out[c] = cX[c] + s[c] / wsum;
}

// (a) step 1 into plane (W*H float4) and step 2 into tile_max (tiles_x * tiles_y float4 {v, l, 0}): one workgroup per tile, or
// for k <= 8 a group of lanes per tile.
hipError_t launch_mblur_pack_tile_max(const MotionBlurArgs& a, const float* motion, const float* depth, float4* plane, float4* tile_max, hipStream_t stream);
// (b) step 3: neighbour_max (tiles_x * tiles_y float4) from tile_max.
hipError_t launch_mblur_neighbour_max(const MotionBlurArgs& a, const float4* tile_max, float4* neighbour_max, hipStream_t stream);
// (c) steps 4 and 5, one thread per pixel.  rgb8 and radiance_out may be null and must not overlap radiance.
hipError_t launch_mblur_gather(const MotionBlurArgs& a, const float4* plane, const float4* neighbour_max, const float* radiance, unsigned char* rgb8,
                               float* radiance_out, hipStream_t stream);

} // namespace ff
