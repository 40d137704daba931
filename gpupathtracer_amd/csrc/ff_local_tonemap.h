// ff_local_tonemap.h — the bilateral-grid local tone mapping behind ff_local_tonemap: a W x H radiance image gives the image in
// which the large-scale (base) log-luminance is compressed about a pivot and the detail on top of it is kept or boosted.  The base
// comes from a bilateral grid (J. Chen, S. Paris, F. Durand, "Real-time edge-aware image processing with the bilateral grid", 2007):
// pixels are added into cells of s x s pixels x one stop, the grid is blurred and every pixel reads it back at its own place AND
// its own luminance, so a strong luminance edge throws no halo.  The per-pixel and per-cell functions of steps 1 to 5 are inline and
// compiled for the host and the device alike: the kernels (ff_local_tonemap.hip) and the host twins ff_local_tonemap_host and
// ff_local_tonemap_grid_host (ff_local_tonemap_api.cpp) call the same code.  The operator is spelled out in
// include/firefly/ff_api.h.
//
// Arithmetic: float32 + - * / and floor, integer operations on a float's bit pattern, every expression evaluated as parenthesised
// below, no fused multiply-add (the library is built with -ffp-contract=off), true divisions.  log, exp and pow appear nowhere, and
// the splat adds integers, so the sides agree bit for bit whatever the order of the adds.
//
// Not offered: a multi-GPU twin, the call folded into ff_display, a bin other than one stop, temporal smoothing of the grid.
#pragma once

#include "../../include/firefly/ff_types.h"

#include "ff_pixel.h"

namespace ff {

constexpr int kLtmBins = 40;                     // bins of one stop: 2^-16 .. 2^24
constexpr int kLtmBinBias = 16;                  // bin = (q10 >> 10) + 16
constexpr int kLtmQ16Min = -16 * 65536;          // the pseudo-log's clamp
constexpr int kLtmQ16Max = 24 * 65536 - 1;
constexpr float kLtmFloor = 1.52587890625e-05f;  // 2^-16: ff_display's histogram floor
constexpr float kLtmMaxGain = 32.0f;             // |g| <= 32 stops

// Everything one call needs besides its buffers; passed by value (kernel arguments).  Images are row-major, top row first.
struct LtmArgs {
    int width, height;
    int cell, shift;   // s and log2 s
    int gw, gh;        // the grid: ceil(W / s) x ceil(H / s) columns of kLtmBins cells
    float inv_cell;    // 1 / s (a power of two: multiplying by it is the division)
    float cm1, dm1;    // compression - 1.0f, detail - 1.0f
    float pivot_log;   // P: step 1's Lf of the pivot
    int identity;      // compression == 1 and detail == 1: the call is a copy and builds no grid
};

// One cell of the grid: the count and the sum of q10, as the splat leaves them (int32) and as the blur has them (float).
struct alignas(8) LtmCellI {
    int32_t n, S;
};
struct alignas(8) LtmCellF {
    float n, S;
};

FF_PIXEL_HD uint32_t ltm_bits(float v)
{
    union {
        float f;
        uint32_t u;
    } c;
    c.f = v;
    return c.u;
}

FF_PIXEL_HD float ltm_from_bits(uint32_t u)
{
    union {
        float f;
        uint32_t u;
    } c;
    c.u = u;
    return c.f;
}

// Step 1.  The luminance of a pixel and whether the pixel is mapped ...
FF_PIXEL_HD float ltm_luminance(const float* c) { return (0.2126f * c[0] + 0.7152f * c[1]) + 0.0722f * c[2]; }

FF_PIXEL_HD bool ltm_mapped(const float* c, float l)
{
    return pixel_finite(c[0]) && pixel_finite(c[1]) && pixel_finite(c[2]) && c[0] >= 0.f && c[1] >= 0.f && c[2] >= 0.f && l >= kLtmFloor && pixel_finite(l);
}

// ... and the piecewise-linear log2 of a finite l >= 2^-16 in 16.16 fixed point, clamped.
FF_PIXEL_HD int ltm_q16(float l)
{
    const uint32_t b = ltm_bits(l);
    const int e = (int)(b >> 23) - 127;
    const int m = (int)(b & 0x7FFFFFu);
    const int q = e * 65536 + (m >> 7);
    return q < kLtmQ16Min ? kLtmQ16Min : (q > kLtmQ16Max ? kLtmQ16Max : q);
}

FF_PIXEL_HD int ltm_q10(int q16) { return q16 >> 6; } // (arithmetic: floor)
FF_PIXEL_HD int ltm_bin(int q10) { return (q10 >> 10) + kLtmBinBias; }
FF_PIXEL_HD float ltm_lf(int q16) { return (float)q16 * 1.52587890625e-05f; } // exact

// Step 3: one tap of the [1 2 1] / 4 blur; a tap outside the grid is 0.0f.
FF_PIXEL_HD float ltm_blur3(float a, float b, float c) { return ((a + (2.0f * b)) + c) * 0.25f; }

// Step 4.  A coordinate clamped into 0 .. last, its cell, the next one and the weight of the next one.
FF_PIXEL_HD void ltm_axis(float f, int last, int& i0, int& i1, float& t)
{
    const float hi = (float)last;
    f = f < 0.0f ? 0.0f : (f > hi ? hi : f);
    const float fl = floorf(f);
    i0 = (int)fl;
    i1 = i0 + 1 > last ? last : i0 + 1;
    t = f - fl;
}

FF_PIXEL_HD float ltm_lerp(float a, float b, float t) { return (a * (1.0f - t)) + (b * t); }

// The base of the mapped pixel (x, y) with log-luminance lf, out of the blurred grid.
FF_PIXEL_HD float ltm_slice(const LtmArgs& a, const LtmCellF* grid, int x, int y, float lf)
{
    int x0, x1, y0, y1, z0, z1;
    float tx, ty, tz;
    ltm_axis((((float)x + 0.5f) * a.inv_cell) - 0.5f, a.gw - 1, x0, x1, tx);
    ltm_axis((((float)y + 0.5f) * a.inv_cell) - 0.5f, a.gh - 1, y0, y1, ty);
    ltm_axis((lf + 16.0f) - 0.5f, kLtmBins - 1, z0, z1, tz);
    const size_t r0 = (size_t)y0 * (size_t)a.gw, r1 = (size_t)y1 * (size_t)a.gw;
    const size_t c00 = (r0 + (size_t)x0) * kLtmBins, c10 = (r0 + (size_t)x1) * kLtmBins;
    const size_t c01 = (r1 + (size_t)x0) * kLtmBins, c11 = (r1 + (size_t)x1) * kLtmBins;
    // the eight taps: (x, y, z) with x fastest in the names below
    const LtmCellF v000 = grid[c00 + z0], v100 = grid[c10 + z0], v010 = grid[c01 + z0], v110 = grid[c11 + z0];
    const LtmCellF v001 = grid[c00 + z1], v101 = grid[c10 + z1], v011 = grid[c01 + z1], v111 = grid[c11 + z1];
    // along x, then y, then z
    const float n00 = ltm_lerp(v000.n, v100.n, tx), n10 = ltm_lerp(v010.n, v110.n, tx);
    const float n01 = ltm_lerp(v001.n, v101.n, tx), n11 = ltm_lerp(v011.n, v111.n, tx);
    const float S00 = ltm_lerp(v000.S, v100.S, tx), S10 = ltm_lerp(v010.S, v110.S, tx);
    const float S01 = ltm_lerp(v001.S, v101.S, tx), S11 = ltm_lerp(v011.S, v111.S, tx);
    const float n0 = ltm_lerp(n00, n10, ty), n1 = ltm_lerp(n01, n11, ty);
    const float S0 = ltm_lerp(S00, S10, ty), S1 = ltm_lerp(S01, S11, ty);
    const float n = ltm_lerp(n0, n1, tz), S = ltm_lerp(S0, S1, tz);
    return n > 0.0f ? (S / n) * 9.765625e-04f : lf; // 2^-10
}

// Step 5: the ratio of a mapped pixel; false where g == 0 (the pixel is copied through).
FF_PIXEL_HD bool ltm_ratio(const LtmArgs& a, float lf, float base, float& ratio)
{
    float g = (a.cm1 * (base - a.pivot_log)) + (a.dm1 * (lf - base));
    g = g < -kLtmMaxGain ? -kLtmMaxGain : (g > kLtmMaxGain ? kLtmMaxGain : g);
    if (g == 0.0f) return false;
    const float k = floorf(g);
    const float f = g - k;
    ratio = (1.0f + f) * ltm_from_bits((uint32_t)((int)k + 127) << 23);
    return true;
}

// Steps 1, 4 and 5 for pixel (x, y) with its radiance: out[3].
FF_PIXEL_HD void ltm_pixel(const LtmArgs& a, const LtmCellF* grid, int x, int y, const float* rad, float* out)
{
    out[0] = rad[0];
    out[1] = rad[1];
    out[2] = rad[2];
    if (a.identity) return;
    const float l = ltm_luminance(rad);
    if (!ltm_mapped(rad, l)) return;
    const float lf = ltm_lf(ltm_q16(l));
    const float base = ltm_slice(a, grid, x, y, lf);
    float ratio;
    if (!ltm_ratio(a, lf, base, ratio)) return;
    out[0] = rad[0] * ratio;
    out[1] = rad[1] * ratio;
    out[2] = rad[2] * ratio;
}

// The kernels (ff_local_tonemap.hip).  `work` holds two grids of gw * gh * kLtmBins cells of 8 bytes; the blurred grid ends up in
// the second.  rgb8 and radiance_out may be null; radiance_out may be radiance itself.
size_t ltm_grid_cells(const LtmArgs& a);
hipError_t launch_local_tonemap(const LtmArgs& a, const float* radiance, void* work, unsigned char* rgb8, float* radiance_out, hipStream_t stream);

} // namespace ff
