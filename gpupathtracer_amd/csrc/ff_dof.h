// ff_dof.h — the gather depth-of-field filter behind ff_depth_of_field: a W x H radiance image and ff_gbuffer's position and depth
// planes give the image every pixel of which is spread over its circle of confusion, the in-path thin lens (ff_camera.h) as a post
// filter on a pinhole frame.  The per-pixel functions of steps 1, 3 and 4 are inline and compiled for the host and the device alike:
// the kernels (ff_dof.hip) and the host twin ff_depth_of_field_host (ff_dof_api.cpp) call the same code.  The operator is spelled
// out in include/firefly/ff_api.h.
//
// Arithmetic: float32 throughout, every expression evaluated as parenthesised below, no fused multiply-add (the library is built
// with -ffp-contract=off), true divisions and square roots (correctly rounded on the device under the library's flags).  exp, pow
// and trigonometry appear nowhere, so the two sides agree bit for bit.
//
// Not offered: a separate near-field layer with background reconstruction, polygonal or anamorphic apertures, bokeh highlights,
// autofocus, a multi-GPU twin.
#pragma once

#include <float.h>
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include <hip/hip_runtime.h>

#include "../../include/firefly/ff_types.h"

#if defined(__HIPCC__)
#define FF_DOF_HD __host__ __device__ __forceinline__
#else
#define FF_DOF_HD inline
#endif

namespace ff {

constexpr int kDofMaxGrid = 8;                    // g <= 8: at most 17 grid columns
constexpr int kDofColumns = 2 * kDofMaxGrid + 1;
constexpr float kDofMinDepth = 1.0e-6f;           // an axial depth at or below this is a miss

// Everything one call needs besides its buffers; passed by value (kernel arguments).  Images are row-major, top row first.
struct DofArgs {
    int width, height;
    int k;                // max_radius: the largest radius and the tile edge
    int g;                // grid
    int tiles_x, tiles_y; // ceil(width / k), ceil(height / k)
    float fi;             // 1 / focus_distance, formed once
    float coc_scale;
    float depth_extent;
    float origin[3];      // m_position
    float forward[3];     // m_forward as the caller's floats
};

FF_DOF_HD bool dof_finite(float v) { return fabsf(v) <= 3.402823466e+38f; } // (false for NaN)

FF_DOF_HD float dof_clamp01(float v) { return v < 0.f ? 0.f : (v > 1.f ? 1.f : v); }

FF_DOF_HD unsigned char dof_u8(float v)
{
    // the project's 8-bit rule (truncation, out-of-range values clamped): ff_k_shade.h to_u8
    const float s = v * 255.0f;
    if (!(s > 0.0f)) return 0;
    if (s >= 255.0f) return 255;
    return (unsigned char)s;
}

// Step 1 for one pixel: {l, zk} from its world position and its depth.
FF_DOF_HD float2 dof_pack(const DofArgs& a, float px, float py, float pz, float depth)
{
    const float ex = px - a.origin[0], ey = py - a.origin[1], ez = pz - a.origin[2];
    const float z = (ex * a.forward[0] + ey * a.forward[1]) + ez * a.forward[2];
    const bool hit = dof_finite(depth) && depth > 0.f && dof_finite(z) && z > kDofMinDepth;
    const float iz = hit ? 1.f / z : 0.f;
    float l = a.coc_scale * fabsf(a.fi - iz);
    if (l > (float)a.k) l = (float)a.k;
    return make_float2(l, hit ? z : FLT_MAX);
}

// Step 3 for tile (tx, ty): the largest T over the 3x3 tiles around it that exist.
FF_DOF_HD float dof_neighbour_max(const DofArgs& a, const float* tile_max, int tx, int ty)
{
    float best = 0.f;
    for (int dy = -1; dy <= 1; ++dy)
        for (int dx = -1; dx <= 1; ++dx) {
            const int qx = tx + dx, qy = ty + dy;
            if (qx < 0 || qy < 0 || qx >= a.tiles_x || qy >= a.tiles_y) continue;
            const float t = tile_max[(size_t)qy * (size_t)a.tiles_x + (size_t)qx];
            best = t > best ? t : best;
        }
    return best;
}

// Step 4's hash of pixel (x, y): ff_motion_blur's.
FF_DOF_HD uint32_t dof_hash(int x, int y)
{
    uint32_t h = ((uint32_t)x * 0x9E3779B1u) ^ ((uint32_t)y * 0x85EBCA77u);
    h ^= h >> 15;
    h *= 0x2C1B3C6Du;
    h ^= h >> 12;
    return h;
}

FF_DOF_HD float dof_u24(uint32_t h) { return (float)(h >> 8) * 5.9604644775390625e-08f - 0.5f; } // 2^-24; [-0.5, 0.5)

// The offset in pixels of grid coordinate i (-g .. g) under jitter j and neighbourhood radius n; |offset| <= 1.5 * 64 = 96.
FF_DOF_HD int dof_offset(float n, int i, float j, int g) { return (int)floorf(n * (((float)i + j) / (float)g) + 0.5f); }

FF_DOF_HD float dof_cover(float d, float l) { return dof_clamp01((l - d) + 0.5f); }

FF_DOF_HD float dof_intensity(float l)
{
    const float q = l > 0.5f ? l : 0.5f;
    return 1.f / (q * q);
}

// Step 4 for pixel (x, y) into out[3].  plane: step 1's {l, zk} per pixel; n: N of the pixel's tile.  The 2g + 1 column offsets do
// not depend on the tap's row: they are formed once into dxs[i * stride], i = 0 .. 2g, the caller's room for them (the kernel's
// is in LDS, one column of bytes per thread; the host's a local array).
FF_DOF_HD void dof_gather(const DofArgs& a, int x, int y, const float2* plane, const float* radiance, float n, signed char* dxs, int stride, float* out)
{
    const size_t X = (size_t)y * (size_t)a.width + (size_t)x;
    const float cX[3] = { radiance[3 * X], radiance[3 * X + 1], radiance[3 * X + 2] };
    out[0] = cX[0];
    out[1] = cX[1];
    out[2] = cX[2];
    if (n <= 0.5f || !(dof_finite(cX[0]) && dof_finite(cX[1]) && dof_finite(cX[2]))) return;
    const float2 pX = plane[X];
    const float lX = pX.x, zX = pX.y;
    const uint32_t h = dof_hash(x, y);
    const float jx = dof_u24(h), jy = dof_u24(h * 0x9E3779B1u);
    const int g = a.g;
    for (int i = -g; i <= g; ++i) dxs[(i + g) * stride] = (signed char)dof_offset(n, i, jx, g);
    float asum = 0.f, s[3] = { 0.f, 0.f, 0.f };
    for (int b = -g; b <= g; ++b) {
        const int dy = dof_offset(n, b, jy, g);
        const int qy = y + dy;
        const int room = g * g - b * b; // the grid point (a, b) is a tap when a * a <= room
        for (int i = -g; i <= g; ++i) {
            if (i * i > room) continue;
            const int dx = dxs[(i + g) * stride];
            const int qx = x + dx;
            if ((dx == 0 && dy == 0) || qx < 0 || qy < 0 || qx >= a.width || qy >= a.height) continue;
            const size_t Y = (size_t)qy * (size_t)a.width + (size_t)qx;
            const float cY[3] = { radiance[3 * Y], radiance[3 * Y + 1], radiance[3 * Y + 2] };
            if (!(dof_finite(cY[0]) && dof_finite(cY[1]) && dof_finite(cY[2]))) continue;
            const float2 pY = plane[Y];
            const float lY = pY.x, zY = pY.y;
            const float d = sqrtf((float)(dx * dx + dy * dy));
            const float f = dof_clamp01(1.f - (zY - zX) / a.depth_extent);
            const float m = lY < lX ? lY : lX;
            const float w = (f * dof_cover(d, lY) + (1.f - f) * dof_cover(d, m)) * dof_intensity(lY);
            s[0] = s[0] + w * (cY[0] - cX[0]);
            s[1] = s[1] + w * (cY[1] - cX[1]);
            s[2] = s[2] + w * (cY[2] - cX[2]);
            asum = asum + w;
        }
    }
    const float wsum = dof_intensity(lX) + asum;
    // (a channel whose sum is 0 keeps the centre's bits: cX + 0 would turn -0 into +0)
    for (int c = 0; c < 3; ++c)
        if (s[c] != 0.f) out[c] = cX[c] + s[c] / wsum;
}

// (a) step 1 into plane (W*H float2) and step 2 into tile_max (tiles_x * tiles_y floats): one workgroup per tile, or for k <= 8 a
// group of lanes per tile.
hipError_t launch_dof_pack_tile_max(const DofArgs& a, const float* position, const float* depth, float2* plane, float* tile_max, hipStream_t stream);
// (b) step 3: neighbour_max (tiles_x * tiles_y floats) from tile_max.
hipError_t launch_dof_neighbour_max(const DofArgs& a, const float* tile_max, float* neighbour_max, hipStream_t stream);
// (c) steps 4 and 5, one thread per pixel.  rgb8 and radiance_out may be null and must not overlap radiance.
hipError_t launch_dof_gather(const DofArgs& a, const float2* plane, const float* neighbour_max, const float* radiance, unsigned char* rgb8,
                             float* radiance_out, hipStream_t stream);

} // namespace ff
