// ff_adaptive.h — the error estimate behind ff_render_adaptive: the stopping condition of Dammertz et al., "A Hierarchical Automatic
// Stopping Condition for Monte Carlo Global Illumination" (2010), on a fixed grid of tiles (the paper's block splitting is left out).
// After n passes, n even, a pixel's error is the distance between the mean of all its passes and the mean of its even passes over
// the square root of its brightness; a tile's error is the sum over its pixels, scaled by the tile's share of the image.  The
// per-pixel function, the fixed order of the sum and the scale are inline and compiled for the host and the device alike: the kernel
// (ff_adaptive.hip) and the host twin ff_adaptive_tile_error_host (ff_adaptive_api.cpp) call the same code.  The operator is spelled
// out in include/firefly/ff_api.h.
//
// Arithmetic: float32 throughout, only + - * / sqrt and fabs, every expression evaluated as parenthesised below, no fused
// multiply-add (the library is built with -ffp-contract=off), correctly rounded divisions and square roots on both sides.  The sum
// over a tile is the one place where an order matters, and the order is part of the definition (adaptive_lane_sum, adaptive_tree):
// it does not depend on the launch shape.
//
// A NaN error is not below any threshold: such a tile stays active until max_passes.
//
// Not offered: the paper's hierarchical block splitting, a pixel-buffer twin, a multi-GPU twin.
#pragma once

#include "../../include/firefly/ff_types.h"

#include "ff_tile_filter.h"

namespace ff {

constexpr int kAdaptiveLanes = 256;       // the lanes of the sum's fixed order: a workgroup of the kernel
constexpr int kAdaptiveMaxPasses = 65534; // (a pixel's pass count leaves as a uint16)

// Everything the error kernel needs besides its buffers; passed by value (kernel arguments).
struct AdaptiveArgs {
    TileGrid grid;      // the image and its tiles (ff_tile_filter.h: row-major tiles, narrower and shorter at the right and bottom edges)
    float inv_n, inv_h; // 1 / n and 1 / (n / 2)
    float image_pixels; // (float)(W * H)
};

inline AdaptiveArgs make_adaptive_args(int width, int height, int tile, int n)
{
    return { make_tile_grid(width, height, tile), 1.0f / (float)n, 1.0f / (float)(n / 2), (float)((uint64_t)width * (uint64_t)height) };
}

inline bool adaptive_tile_ok(int tile) { return tile == 16 || tile == 32 || tile == 64 || tile == 128; }

// The pixels of tile (tx, ty).
FF_PIXEL_HD int adaptive_tile_pixels(const TileGrid& g, int tx, int ty)
{
    const int x0 = tx * g.k, y0 = ty * g.k;
    const int tw = g.k < g.width - x0 ? g.k : g.width - x0, th = g.k < g.height - y0 ? g.k : g.height - y0;
    return tw * th;
}

// e_p of the pixel whose three running sums over all of its passes and over its even passes are given.
FF_PIXEL_HD float adaptive_pixel_error(const float* sum, const float* sum_even, float inv_n, float inv_h)
{
    const float ir = sum[0] * inv_n, ig = sum[1] * inv_n, ib = sum[2] * inv_n;
    const float ar = sum_even[0] * inv_h, ag = sum_even[1] * inv_h, ab = sum_even[2] * inv_h;
    const float d = (ir + ig) + ib;
    if (!(d > 0.f)) return 0.f;
    return ((fabsf(ir - ar) + fabsf(ig - ag)) + fabsf(ib - ab)) / sqrtf(d);
}

// What lane `lane` of kAdaptiveLanes holds before the tree: e_lane + e_(lane + 256) + ... in that order, from 0.0f.
FF_PIXEL_HD float adaptive_lane_sum(const AdaptiveArgs& a, int tx, int ty, int lane, const float* sum, const float* sum_even)
{
    float v = 0.0f;
    size_t p;
    for (int i = lane; tile_pixel(a.grid, tx, ty, i, &p); i += kAdaptiveLanes) v = v + adaptive_pixel_error(sum + 3 * p, sum_even + 3 * p, a.inv_n, a.inv_h);
    return v;
}

// E_t from the tree's result S and the tile's pixel count.
FF_PIXEL_HD float adaptive_tile_scale(const AdaptiveArgs& a, float S, int tile_pixels)
{
    const float n_t = (float)tile_pixels;
    return S * sqrtf(n_t / a.image_pixels) / n_t;
}

// The halving tree on the host: v[j] += v[j + off] for off = 128, 64, ..., 1 (the kernel runs the same steps in LDS).
inline float adaptive_tree(float* v)
{
    for (int off = kAdaptiveLanes / 2; off >= 1; off >>= 1)
        for (int j = 0; j < off; ++j) v[j] = v[j] + v[j + off];
    return v[0];
}

// The kernels (ff_adaptive.hip).  work is a compact w x h x 3 rectangle that lands at (x0, y0) of the width-wide planes; `first`:
// the pass is number 0 (the sums are written, not added to), `even`: the pass also counts for sum_even.
hipError_t launch_adaptive_accumulate(float* sum, float* sum_even, const float* work, int width, int x0, int y0, int w, int h, int first, int even,
                                      hipStream_t stream);
// E_t of the `count` tiles listed in `tiles` (row-major tile indices; null: tiles 0 .. count - 1) into tile_error[tile].
hipError_t launch_adaptive_tile_error(const AdaptiveArgs& a, const float* sum, const float* sum_even, const uint32_t* tiles, int count, float* tile_error,
                                      hipStream_t stream);
// radiance = sum * (1 / n_t), rgb8 = the project's 8-bit rule of it, passes = n_t; each output may be null.
hipError_t launch_adaptive_resolve(const TileGrid& grid, const float* sum, const uint16_t* tile_passes, float* radiance, unsigned char* rgb8, uint16_t* passes,
                                   hipStream_t stream);

} // namespace ff
