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

#include "../../include/firefly/ff_types.h"
#include "ff_tile_filter.h"

namespace ff {

constexpr int kDofMaxGrid = 8;                    // g <= 8: at most 17 grid columns
constexpr int kDofColumns = 2 * kDofMaxGrid + 1;
constexpr float kDofMinDepth = 1.0e-6f;           // an axial depth at or below this is a miss

// Everything one call needs besides its buffers; passed by value (kernel arguments).  Images are row-major, top row first.
struct DofArgs {
    TileGrid grid;        // k = max_radius: the largest radius and the tile edge
    int g;                // grid
    float fi;             // 1 / focus_distance, formed once
    float coc_scale;
    float depth_extent;
    float origin[3];      // m_position
    float forward[3];     // m_forward as the caller's floats
};

// Step 1 for one pixel: {l, zk} from its world position and its depth.
FF_PIXEL_HD float2 dof_pack(const DofArgs& a, float px, float py, float pz, float depth)
{
    const float ex = px - a.origin[0], ey = py - a.origin[1], ez = pz - a.origin[2];
    const float z = (ex * a.forward[0] + ey * a.forward[1]) + ez * a.forward[2];
    const bool hit = pixel_finite(depth) && depth > 0.f && pixel_finite(z) && z > kDofMinDepth;
    const float iz = hit ? 1.f / z : 0.f;
    float l = a.coc_scale * fabsf(a.fi - iz);
    if (l > (float)a.grid.k) l = (float)a.grid.k;
    return make_float2(l, hit ? z : FLT_MAX);
}

// Step 3 for tile (tx, ty): the largest T over the 3x3 tiles around it that exist.
FF_PIXEL_HD float dof_neighbour_max(const DofArgs& a, const float* tile_max, int tx, int ty)
{
    float best = 0.f;
    for (int dy = -1; dy <= 1; ++dy)
        for (int dx = -1; dx <= 1; ++dx) {
            const int qx = tx + dx, qy = ty + dy;
            if (qx < 0 || qy < 0 || qx >= a.grid.tiles_x || qy >= a.grid.tiles_y) continue;
            const float t = tile_max[(size_t)qy * (size_t)a.grid.tiles_x + (size_t)qx];
            best = t > best ? t : best;
        }
    return best;
}

// The offset in pixels of grid coordinate i (-g .. g) under jitter j and neighbourhood radius n; |offset| <= 1.5 * 64 = 96.
FF_PIXEL_HD int dof_offset(float n, int i, float j, int g) { return (int)floorf(n * (((float)i + j) / (float)g) + 0.5f); }

FF_PIXEL_HD float dof_cover(float d, float l) { return pixel_clamp01((l - d) + 0.5f); }

FF_PIXEL_HD float dof_intensity(float l)
{
    const float q = l > 0.5f ? l : 0.5f;
    return 1.f / (q * q);
}

// Step 4 for pixel (x, y) into out[3].  plane: step 1's {l, zk} per pixel; n: N of the pixel's tile.  The 2g + 1 column offsets do
// not depend on the tap's row: they are formed once into dxs[i * stride], i = 0 .. 2g, the caller's room for them (the kernel's
// is in LDS, one column of bytes per thread; the host's a local array).
FF_PIXEL_HD void dof_gather(const DofArgs& a, int x, int y, const float2* plane, const float* radiance, float n, signed char* dxs, int stride, float* out)
{
    const size_t X = (size_t)y * (size_t)a.grid.width + (size_t)x;
    const float cX[3] = { radiance[3 * X], radiance[3 * X + 1], radiance[3 * X + 2] };
    out[0] = cX[0];
    out[1] = cX[1];
    out[2] = cX[2];
    if (n <= 0.5f || !(pixel_finite(cX[0]) && pixel_finite(cX[1]) && pixel_finite(cX[2]))) return;
    const float2 pX = plane[X];
    const float lX = pX.x, zX = pX.y;
    const uint32_t h = pixel_hash(x, y);
    const float jx = pixel_u24(h), jy = pixel_u24(h * 0x9E3779B1u);
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
            if ((dx == 0 && dy == 0) || qx < 0 || qy < 0 || qx >= a.grid.width || qy >= a.grid.height) continue;
            const size_t Y = (size_t)qy * (size_t)a.grid.width + (size_t)qx;
            const float cY[3] = { radiance[3 * Y], radiance[3 * Y + 1], radiance[3 * Y + 2] };
            if (!(pixel_finite(cY[0]) && pixel_finite(cY[1]) && pixel_finite(cY[2]))) continue;
            const float2 pY = plane[Y];
            const float lY = pY.x, zY = pY.y;
            const float d = sqrtf((float)(dx * dx + dy * dy));
            const float f = pixel_clamp01(1.f - (zY - zX) / a.depth_extent);
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

// What ff_tile_filter.h needs to know of the filter.  T is the tile's largest l, and so is the key: finite and >= 0, a plain float
// maximum that can tie, written by one lane.
struct DofFilter {
    using Args = DofArgs;
    using Packed = float2;
    using Tile = float;
    using Key = float;
    static constexpr int kGuideFloats = 3, kGatherRoom = kDofColumns;
    static constexpr bool kUniqueKey = false;
    FF_PIXEL_HD static Key lowest_key() { return 0.f; } // (no radius)
    FF_PIXEL_HD static Packed pack(const Args& a, const float* position, float depth) { return dof_pack(a, position[0], position[1], position[2], depth); }
    FF_PIXEL_HD static Key key(const Packed& v, unsigned) { return v.x; }
    FF_PIXEL_HD static Tile tile_of(const Packed& v) { return v.x; }
    FF_PIXEL_HD static Tile neighbour_max(const Args& a, const Tile* tile_max, int tx, int ty) { return dof_neighbour_max(a, tile_max, tx, ty); }
    FF_PIXEL_HD static void gather(const Args& a, int x, int y, const Packed* plane, const float* radiance, Tile n, signed char* dxs, int stride, float* out)
    {
        dof_gather(a, x, y, plane, radiance, n, dxs, stride, out);
    }
    // (c) steps 4 and 5 (ff_dof.hip).  rgb8 and radiance_out may be null and must not overlap radiance.
    static hipError_t launch_gather(const Args& a, const Packed* plane, const Tile* neighbour_max, const float* radiance, unsigned char* rgb8,
                                    float* radiance_out, hipStream_t stream);
};

} // namespace ff
