// ff_yuv.h — the Y'CbCr 4:2:0 encoding behind ff_encode_yuv: a W x H image of display-linear float3 gives the NV12 (8-bit) or P010
// (10-bit) planes a video encoder takes.  The per-pixel functions of steps 1 to 5 and the per-sample functions of steps 6 and 7 are
// inline and compiled for the host and the device alike: the kernel (ff_yuv.hip) and the host twin ff_encode_yuv_host
// (ff_yuv_api.cpp) call the same code.  The operator is spelled out in include/firefly/ff_api.h.
//
// Arithmetic: float32 throughout, every expression evaluated as parenthesised below, no fused multiply-add (the library is built
// with -ffp-contract=off), true divisions (correctly rounded on the device under the library's flags), floorf.  pow appears only
// where the knots are made, in double on the host, so the two sides agree bit for bit.
//
// Not offered: 4:4:4 and 4:2:2 output, HLG, dithering, top-left (type 2) siting, row pitches other than tight.
#pragma once

#include "../../include/firefly/ff_types.h"

#include "ff_pixel.h"

namespace ff {

constexpr int kYuvCells = 4096;             // the transfer's cells; K_0 .. K_4096 are its kYuvCells + 1 knots
constexpr int kYuvKnots = kYuvCells + 1;
constexpr int kYuvKnotStride = 4112;        // floats between two transfers' tables on the device (a multiple of 16 bytes)
constexpr float kYuvMaxC = 65536.0f;        // step 1's ceiling

// Everything one call needs besides its buffers; passed by value (kernel arguments).  Images are row-major, top row first.
struct YuvArgs {
    int width, height;
    int bt2020;       // FF_YUV_MATRIX_BT2020: step 2 runs and step 5 takes the BT.2020 coefficients
    int pq;           // FF_YUV_TRANSFER_PQ: step 3 scales
    int full;         // FF_YUV_RANGE_FULL
    int depth;        // 8 or 10 (the kernel has it as a template argument)
    int left;         // FF_YUV_SITING_LEFT (the kernel has it as a template argument)
    int vec;          // the kernel's whole-dword paths may run: width is a multiple of 4 and the three buffers are 16-byte aligned
    float scale;      // reference_white_nits / 10000, formed once in float (PQ only)
    const float* knots; // K_0 .. K_4096 of the transfer (the kernel copies them into LDS)
};

// One pixel after step 5: the luma code and the unquantised colour differences.
struct YuvPixel {
    int y;
    float cb, cr;
};

// Step 1 for one channel: NaN and negative values (and -0) become +0, then min(c, 65536).
FF_PIXEL_HD float yuv_sanitise(float c)
{
    if (!(c > 0.f)) return 0.f;
    return c > kYuvMaxC ? kYuvMaxC : c;
}

// Step 4: the piecewise-linear inverse of the EOTF whose knots are K[0 .. 4096]; 0 <= v <= 1.
FF_PIXEL_HD float yuv_transfer(const float* K, float v)
{
    if (v >= 1.0f) return 1.0f;
    int j = 0; // the number of K_1 .. K_4095 that are <= v
#pragma unroll
    for (int step = kYuvCells / 2; step >= 1; step >>= 1)
        if (K[j + step] <= v) j += step;
    const float k0 = K[j], k1 = K[j + 1];
    return ((float)j + (v - k0) / (k1 - k0)) * 0.000244140625f; // 1 / 4096
}

// Step 7 for a luma value and for a colour difference.
template <int DEPTH>
FF_PIXEL_HD int yuv_quant_luma(float y, int full)
{
    constexpr float s = (float)(1 << (DEPTH - 8)), m = (float)((1 << DEPTH) - 1);
    return (int)(full ? floorf(y * m + 0.5f) : floorf((219.0f * y + 16.0f) * s + 0.5f));
}

template <int DEPTH>
FF_PIXEL_HD int yuv_quant_chroma(float c, int full)
{
    constexpr float s = (float)(1 << (DEPTH - 8)), m = (float)((1 << DEPTH) - 1), half = (float)(1 << (DEPTH - 1));
    const float q = full ? floorf((c * m + half) + 0.5f) : floorf((224.0f * c + 128.0f) * s + 0.5f);
    const float lo = full ? 0.f : 16.0f * s, hi = full ? m : 240.0f * s;
    return (int)(q < lo ? lo : (q > hi ? hi : q));
}

// Steps 1 to 5 and the luma half of step 7 for the pixel whose three floats are given.
template <int DEPTH>
FF_PIXEL_HD YuvPixel yuv_pixel(const YuvArgs& a, const float* K, const float* c)
{
    float r = yuv_sanitise(c[0]), g = yuv_sanitise(c[1]), b = yuv_sanitise(c[2]);
    if (a.bt2020) {
        const float r2 = (0.6274f * r + 0.3293f * g) + 0.0433f * b;
        const float g2 = (0.0691f * r + 0.9195f * g) + 0.0114f * b;
        const float b2 = (0.0164f * r + 0.0880f * g) + 0.8956f * b;
        r = r2;
        g = g2;
        b = b2;
    }
    if (a.pq) {
        r = r * a.scale;
        g = g * a.scale;
        b = b * a.scale;
    }
    r = yuv_transfer(K, r > 1.0f ? 1.0f : r);
    g = yuv_transfer(K, g > 1.0f ? 1.0f : g);
    b = yuv_transfer(K, b > 1.0f ? 1.0f : b);
    const float kr = a.bt2020 ? 0.2627f : 0.2126f, kg = a.bt2020 ? 0.6780f : 0.7152f, kb = a.bt2020 ? 0.0593f : 0.0722f;
    const float dcb = a.bt2020 ? 1.8814f : 1.8556f, dcr = a.bt2020 ? 1.4746f : 1.5748f;
    const float y = (kr * r + kg * g) + kb * b;
    YuvPixel o;
    o.y = yuv_quant_luma<DEPTH>(y, a.full);
    o.cb = (b - y) / dcb;
    o.cr = (r - y) / dcr;
    return o;
}

// Step 6 for one plane: CENTER from the 2 x 2 block {c00 c10 / c01 c11}; LEFT from the columns 2X-1, 2X, 2X+1 of the rows 2Y (a*)
// and 2Y+1 (b*).
FF_PIXEL_HD float yuv_chroma_center(float c00, float c10, float c01, float c11) { return ((c00 + c10) + (c01 + c11)) * 0.25f; }

FF_PIXEL_HD float yuv_chroma_left(float am, float a0, float ap, float bm, float b0, float bp)
{
    const float ha = (am * 0.25f + a0 * 0.5f) + ap * 0.25f;
    const float hb = (bm * 0.25f + b0 * 0.5f) + bp * 0.25f;
    return (ha + hb) * 0.5f;
}

// The kernel (ff_yuv.hip): steps 1 to 8 in one launch.  linear_in, luma and chroma are device pointers; a.knots too.
hipError_t launch_encode_yuv(const YuvArgs& a, const float* linear_in, void* luma, void* chroma, hipStream_t stream);

} // namespace ff
