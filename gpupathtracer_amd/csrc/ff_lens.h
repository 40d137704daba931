// ff_lens.h — the gather behind ff_lens: every output pixel of a W x H radiance image computes where in the source each of its
// channels comes from - a radial displacement read from a table over r^2 that the host folds the Brown-Conrady polynomial, the
// direction and the zoom into, times a per-channel magnification (lateral chromatic aberration) - resamples there (bilinear or
// Catmull-Rom, 4 x 4 taps) and multiplies a radial gain in (vignetting).  The per-pixel functions are inline and compiled for the
// host and the device alike: the kernel (ff_lens.hip), the host twin ff_lens_host and ff_lens_map_host (ff_lens_api.cpp) call
// the same code.  The operator is spelled out in include/firefly/ff_api.h.
//
// Arithmetic: float32 throughout, every expression evaluated as parenthesised below, no fused multiply-add (the library is built
// with -ffp-contract=off).  + - * and floor only (no division, no sqrt: r^2 is the tables' axis), so the two sides agree bit for bit.
//
// Not offered: tangential (decentering) terms, fisheye and other projections, filtered minification, a multi-GPU twin.
#pragma once

#include "../../include/firefly/ff_types.h"

#include "ff_pixel.h"

namespace ff {

constexpr int kLensKnots = FF_LENS_KNOTS;
// the kernel's three filter forms (a template argument there)
enum { kLensBilinear = 0, kLensCatmullRom = 1, kLensCatmullRomClamped = 2 };

// One knot of the two tables, side by side so that a pixel reads both with one index: e(r^2) and gain(r^2).
struct LensKnot {
    float e, gain;
};

// Everything one call needs besides its buffers and the table; passed by value (kernel arguments).  Images are row-major, top row
// first.
struct LensArgs {
    int width, height;
    float cx, cy;      // the optical centre in pixels: W/2 + center_x, H/2 + center_y
    float inv_d2;      // 1 / (half the diagonal)^2, pixels^-2
    float knot_scale;  // FF_LENS_KNOTS / r2_max
    float q_red, q_blue;
    int filter;        // kLens* (the kernel has it as a template argument)
    int per_channel;   // either q is nonzero: three positions per pixel (a template argument too)
    int border;        // FF_LENS_BORDER_*
};

// min and max as the header defines them.
FF_PIXEL_HD float lens_min(float a, float b) { return b < a ? b : a; }
FF_PIXEL_HD float lens_max(float a, float b) { return a < b ? b : a; }
// v into [0, hi]; anything that is not > 0 (a NaN too) gives 0
FF_PIXEL_HD float lens_clamp(float v, float hi) { return v > 0.f ? (v < hi ? v : hi) : 0.f; }
FF_PIXEL_HD float lens_value(float v) { return pixel_finite(v) ? v : 0.f; }
FF_PIXEL_HD float lens_lerp(float a, float b, float t) { return a + t * (b - a); }
FF_PIXEL_HD int lens_index(int i, int n) { return i < 0 ? 0 : (i > n - 1 ? n - 1 : i); }

// Catmull-Rom weights of taps -1 .. 2 for fraction t: taa_catmull_rom's expressions (ff_taa_common.h).
FF_PIXEL_HD void lens_catmull_rom(float t, float* w)
{
    const float t2 = t * t, t3 = t2 * t;
    w[0] = ((-t3 + 2.f * t2) - t) * 0.5f;
    w[1] = ((3.f * t3 - 5.f * t2) + 2.f) * 0.5f;
    w[2] = ((-3.f * t3 + 4.f * t2) + t) * 0.5f;
    w[3] = (t3 - t2) * 0.5f;
}

// Step 1: e and gain at the place (px, py) - a pixel centre, or any finite position for ff_lens_map_host.
FF_PIXEL_HD void lens_radial(const LensArgs& a, const LensKnot* table, float px, float py, float& dx, float& dy, float& e, float& gain)
{
    dx = px - a.cx;
    dy = py - a.cy;
    const float r2 = ((dx * dx) + (dy * dy)) * a.inv_d2;
    float u = r2 * a.knot_scale;
    u = u < (float)kLensKnots ? u : (float)kLensKnots; // (a position beyond the last knot reads the last knot)
    int i = (int)floorf(u);
    i = i > kLensKnots - 1 ? kLensKnots - 1 : (i < 0 ? 0 : i);
    const float t = u - (float)i;
    const LensKnot k0 = table[i], k1 = table[i + 1];
    e = lens_lerp(k0.e, k1.e, t);
    gain = lens_lerp(k0.gain, k1.gain, t);
}

// Step 2: the source position of one channel (q: its magnification against green).
FF_PIXEL_HD void lens_source(float px, float py, float dx, float dy, float e, float q, float& sx, float& sy)
{
    const float ec = (e + q) + (e * q);
    sx = px + (dx * ec);
    sy = py + (dy * ec);
}

// Steps 3 and 4 at source position (sx, sy): N channels starting at channel c0 of the float3 image (N = 3, c0 = 0: the three
// channels share the position; N = 1: channel c0 alone), into out[0 .. N-1].
template <int FILTER, int N>
FF_PIXEL_HD void lens_sample(const LensArgs& a, const float* img, int c0, float sx, float sy, float* out)
{
    const float wf = (float)a.width, hf = (float)a.height;
    const bool inside = sx >= 0.f && sx <= wf && sy >= 0.f && sy <= hf; // (false for NaN)
    if (a.border == FF_LENS_BORDER_BLACK && !inside) {
#pragma unroll
        for (int c = 0; c < N; ++c) out[c] = 0.f;
        return;
    }
    const float ux = lens_clamp(sx, wf) - 0.5f, uy = lens_clamp(sy, hf) - 0.5f;
    const float flx = floorf(ux), fly = floorf(uy);
    const int ix = (int)flx, iy = (int)fly; // -1 .. width - 1, -1 .. height - 1
    const float fx = ux - flx, fy = uy - fly;
    const size_t w = (size_t)a.width;
    if (FILTER == kLensBilinear) {
        const size_t x0 = (size_t)lens_index(ix, a.width), x1 = (size_t)lens_index(ix + 1, a.width);
        const size_t r0 = (size_t)lens_index(iy, a.height) * w, r1 = (size_t)lens_index(iy + 1, a.height) * w;
#pragma unroll
        for (int c = 0; c < N; ++c) {
            const float v00 = lens_value(img[3 * (r0 + x0) + c0 + c]), v10 = lens_value(img[3 * (r0 + x1) + c0 + c]);
            const float v01 = lens_value(img[3 * (r1 + x0) + c0 + c]), v11 = lens_value(img[3 * (r1 + x1) + c0 + c]);
            const float v = lens_lerp(lens_lerp(v00, v10, fx), lens_lerp(v01, v11, fx), fy);
            out[c] = (fx == 0.f && fy == 0.f) ? v00 : v;
        }
    } else {
        float wx[4], wy[4];
        lens_catmull_rom(fx, wx);
        lens_catmull_rom(fy, wy);
        size_t xs[4], rows[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            xs[j] = (size_t)lens_index(ix - 1 + j, a.width);
            rows[j] = (size_t)lens_index(iy - 1 + j, a.height) * w;
        }
#pragma unroll
        for (int c = 0; c < N; ++c) {
            float row[4], lo = 0.f, hi = 0.f, centre = 0.f;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float v[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) v[i] = lens_value(img[3 * (rows[j] + xs[i]) + c0 + c]);
                row[j] = (((wx[0] * v[0]) + (wx[1] * v[1])) + (wx[2] * v[2])) + (wx[3] * v[3]);
                if (j == 1) {
                    centre = v[1];
                    lo = lens_min(v[1], v[2]);
                    hi = lens_max(v[1], v[2]);
                }
                if (j == 2) {
                    lo = lens_min(lens_min(lo, v[1]), v[2]);
                    hi = lens_max(lens_max(hi, v[1]), v[2]);
                }
            }
            float v = (((wy[0] * row[0]) + (wy[1] * row[1])) + (wy[2] * row[2])) + (wy[3] * row[3]);
            if (FILTER == kLensCatmullRomClamped) v = lens_min(lens_max(v, lo), hi);
            out[c] = (fx == 0.f && fy == 0.f) ? centre : v;
        }
    }
}

// Steps 1 to 5 for output pixel (x, y): out[3].
template <int FILTER, bool PER_CHANNEL>
FF_PIXEL_HD void lens_pixel(const LensArgs& a, const LensKnot* table, const float* img, int x, int y, float* out)
{
    const float px = (float)x + 0.5f, py = (float)y + 0.5f;
    float dx, dy, e, gain, sx, sy;
    lens_radial(a, table, px, py, dx, dy, e, gain);
    if (PER_CHANNEL) {
        lens_source(px, py, dx, dy, e, a.q_red, sx, sy);
        lens_sample<FILTER, 1>(a, img, 0, sx, sy, out);
        lens_source(px, py, dx, dy, e, 0.f, sx, sy);
        lens_sample<FILTER, 1>(a, img, 1, sx, sy, out + 1);
        lens_source(px, py, dx, dy, e, a.q_blue, sx, sy);
        lens_sample<FILTER, 1>(a, img, 2, sx, sy, out + 2);
    } else {
        lens_source(px, py, dx, dy, e, 0.f, sx, sy);
        lens_sample<FILTER, 3>(a, img, 0, sx, sy, out);
    }
    out[0] = out[0] * gain;
    out[1] = out[1] * gain;
    out[2] = out[2] * gain;
}

// The kernel (ff_lens.hip): one launch.  `table` holds kLensKnots + 1 knots on the device; rgb8 and radiance_out may be null and
// must not overlap the input.  max_blocks: the most workgroups the launch may have (each loads the table once and walks tiles).
hipError_t launch_lens(const LensArgs& a, const LensKnot* table, const float* radiance, unsigned char* rgb8, float* radiance_out, int max_blocks,
                       hipStream_t stream);

} // namespace ff
