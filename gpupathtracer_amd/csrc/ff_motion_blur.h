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

#include <string.h>

#include "../../include/firefly/ff_types.h"
#include "ff_tile_filter.h"

namespace ff {

// Everything one call needs besides its buffers; passed by value (kernel arguments).  Images are row-major, top row first.
struct MotionBlurArgs {
    TileGrid grid;      // k = max_radius: the longest half-spread and the tile edge
    int samples;        // S
    float half_shutter; // 0.5f * shutter, formed once
    float depth_extent;
};

FF_PIXEL_HD uint32_t mblur_bits(float v)
{
    uint32_t b;
    memcpy(&b, &v, sizeof b);
    return b;
}

// Step 1 for one pixel: {v.x, v.y, l, z} from its motion m and its depth.
FF_PIXEL_HD float4 mblur_pack(const MotionBlurArgs& a, float mx, float my, float depth)
{
    float vx = mx * a.half_shutter, vy = my * a.half_shutter;
    if (!(pixel_finite(vx) && pixel_finite(vy))) vx = vy = 0.f;
    float l = sqrtf(vx * vx + vy * vy);
    if (l > (float)a.grid.k) {
        const float s = (float)a.grid.k / l;
        vx = vx * s;
        vy = vy * s;
        l = sqrtf(vx * vx + vy * vy);
    }
    const float z = (pixel_finite(depth) && depth > 0.f) ? depth : FLT_MAX;
    return make_float4(vx, vy, l, z);
}

// The key of steps 2 and 3: the float bits of the squared length above an inverted index, so that the largest key is the largest
// squared length and, among equals, the smallest index.  (The squared length is >= +0 and finite or +Inf: its bits are ordered.)
FF_PIXEL_HD unsigned long long mblur_key(float vx, float vy, unsigned index)
{
    return ((unsigned long long)mblur_bits(vx * vx + vy * vy) << 32) | (unsigned long long)(0xFFFFFFFFu - index);
}

// Step 3 for tile (tx, ty): the largest T over the 3x3 tiles around it that exist, ties to the first in row-major order.
FF_PIXEL_HD float4 mblur_neighbour_max(const MotionBlurArgs& a, const float4* tile_max, int tx, int ty)
{
    unsigned long long best = 0;
    float4 out = make_float4(0.f, 0.f, 0.f, 0.f);
    unsigned n = 0;
    for (int dy = -1; dy <= 1; ++dy)
        for (int dx = -1; dx <= 1; ++dx, ++n) {
            const int qx = tx + dx, qy = ty + dy;
            if (qx < 0 || qy < 0 || qx >= a.grid.tiles_x || qy >= a.grid.tiles_y) continue;
            const float4 t = tile_max[(size_t)qy * (size_t)a.grid.tiles_x + (size_t)qx];
            const unsigned long long key = mblur_key(t.x, t.y, n);
            if (key > best) {
                best = key;
                out = t;
            }
        }
    return out;
}

FF_PIXEL_HD float mblur_soft(float za, float zb, float extent) { return pixel_clamp01(1.f - (za - zb) / extent); }

FF_PIXEL_HD float mblur_cone(float d, float l) { return l > 0.f ? pixel_clamp01(1.f - d / l) : 0.f; }

FF_PIXEL_HD float mblur_cylinder(float d, float l)
{
    if (!(l > 0.f)) return 0.f;
    const float lo = 0.95f * l, hi = 1.05f * l;
    const float u = pixel_clamp01((d - lo) / (hi - lo));
    return 1.f - ((u * u) * (3.f - (2.f * u)));
}

// Step 4's jitter for pixel (x, y): j in [-0.5, 0.5).
FF_PIXEL_HD float mblur_jitter(int x, int y) { return pixel_u24(pixel_hash(x, y)); }

// Step 4 for pixel (x, y) into out[3].  plane: step 1's {v, l, z} per pixel; n: N of the pixel's tile.
FF_PIXEL_HD void mblur_gather(const MotionBlurArgs& a, int x, int y, const float4* plane, const float* radiance, float4 n, float* out)
{
    const size_t X = (size_t)y * (size_t)a.grid.width + (size_t)x;
    const float cX[3] = { radiance[3 * X], radiance[3 * X + 1], radiance[3 * X + 2] };
    out[0] = cX[0];
    out[1] = cX[1];
    out[2] = cX[2];
    if (n.z <= 0.5f || !(pixel_finite(cX[0]) && pixel_finite(cX[1]) && pixel_finite(cX[2]))) return;
    const float4 pX = plane[X];
    const float lX = pX.z, zX = pX.w;
    const float j = mblur_jitter(x, y);
    const float steps = (float)(a.samples + 1);
    float asum = 0.f, s[3] = { 0.f, 0.f, 0.f };
    for (int i = 0; i < a.samples; ++i) {
        const float t = ((((float)i + j) + 1.f) / steps) * 2.f - 1.f;
        const int dx = (int)floorf(n.x * t + 0.5f), dy = (int)floorf(n.y * t + 0.5f);
        const int qx = x + dx, qy = y + dy;
        if ((dx == 0 && dy == 0) || qx < 0 || qy < 0 || qx >= a.grid.width || qy >= a.grid.height) continue;
        const size_t Y = (size_t)qy * (size_t)a.grid.width + (size_t)qx;
        const float cY[3] = { radiance[3 * Y], radiance[3 * Y + 1], radiance[3 * Y + 2] };
        if (!(pixel_finite(cY[0]) && pixel_finite(cY[1]) && pixel_finite(cY[2]))) continue;
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

// What ff_tile_filter.h needs to know of the filter.  T is {v, l, 0}; the key is unique in a tile.
struct MotionBlurFilter {
    using Args = MotionBlurArgs;
    using Packed = float4;
    using Tile = float4;
    using Key = unsigned long long;
    static constexpr int kGuideFloats = 2, kGatherRoom = 0;
    static constexpr bool kUniqueKey = true;
    FF_PIXEL_HD static Key lowest_key() { return 0; } // (every pixel's key is above 0: its low word is at least 2^32 - 4096)
    FF_PIXEL_HD static Packed pack(const Args& a, const float* motion, float depth) { return mblur_pack(a, motion[0], motion[1], depth); }
    FF_PIXEL_HD static Key key(const Packed& v, unsigned index) { return mblur_key(v.x, v.y, index); }
    FF_PIXEL_HD static Tile tile_of(const Packed& v) { return make_float4(v.x, v.y, v.z, 0.f); }
    FF_PIXEL_HD static Tile neighbour_max(const Args& a, const Tile* tile_max, int tx, int ty) { return mblur_neighbour_max(a, tile_max, tx, ty); }
    FF_PIXEL_HD static void gather(const Args& a, int x, int y, const Packed* plane, const float* radiance, Tile n, signed char*, int, float* out)
    {
        mblur_gather(a, x, y, plane, radiance, n, out);
    }
    // (c) steps 4 and 5 (ff_motion_blur.hip).  rgb8 and radiance_out may be null and must not overlap radiance.
    static hipError_t launch_gather(const Args& a, const Packed* plane, const Tile* neighbour_max, const float* radiance, unsigned char* rgb8,
                                    float* radiance_out, hipStream_t stream);
};

} // namespace ff
