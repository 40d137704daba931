// ff_sharpen.h — the contrast-adaptive sharpening behind ff_sharpen: a W x H radiance image gives the image in which every pixel
// is pushed away from the mean of its four cross neighbours, by a negative lobe that is limited per pixel so that the result stays
// inside the neighbours' range (it cannot ring), in a range-compressed domain c / (1 + max c) so that an HDR highlight throws no
// dark halo.  The per-pixel functions of steps 1 to 5 are inline and compiled for the host and the device alike: the kernel
// (ff_sharpen.hip) and the host twin ff_sharpen_host (ff_sharpen_api.cpp) call the same code.  The operator is spelled out in
// include/firefly/ff_api.h.
//
// Arithmetic: float32 throughout, every expression evaluated as parenthesised below, no fused multiply-add (the library is built
// with -ffp-contract=off), true divisions (correctly rounded on the device under the library's flags).  exp, pow and sqrt appear
// nowhere, so the two sides agree bit for bit.
//
// Not offered: the 3 x 3 (9-tap) form, sharpening inside ff_taa_upscale's kernel, a G-buffer-guided form, a multi-GPU twin.
#pragma once

#include "../../include/firefly/ff_types.h"

#include "ff_pixel.h"

namespace ff {

constexpr float kSharpenLimit = 0.1875f;    // LIMIT: the deepest lobe
constexpr float kSharpenCap = 0.99999988f;  // CAP = 1 - 2^-23: the largest compressed value
constexpr float kSharpenMaxC = 8388608.0f;  // MAXC = 2^23: the largest channel of a usable pixel (1 + m is exact up to here)

// Everything one call needs besides its buffers; passed by value (kernel arguments).  Images are row-major, top row first.
struct SharpenArgs {
    int width, height;
    float strength;
    int noise_aware; // FF_SHARPEN_NOISE_AWARE (the kernel has it as a template argument)
};

// Step 1's result for one pixel: the compressed channels and their luminance.  l >= 0 for a usable pixel; the two marks below
// stand in l otherwise, so that step 2's rule needs no second plane.
struct alignas(16) SharpenCell {
    float t[3];
    float l;
};
constexpr float kSharpenUnusable = -1.f; // the pixel is not usable: whoever has it in its cross is copied through
constexpr float kSharpenOutside = -2.f;  // the cell lies outside the image: the tap is E itself

// min and max as the header defines them (a NaN never reaches them; neither does a pair of zeros of different sign).
FF_PIXEL_HD float sharpen_min(float a, float b) { return b < a ? b : a; }
FF_PIXEL_HD float sharpen_max(float a, float b) { return a < b ? b : a; }

// Step 1 for the pixel whose three radiance floats are given.
FF_PIXEL_HD SharpenCell sharpen_compress(const float* c)
{
    SharpenCell s;
    s.t[0] = s.t[1] = s.t[2] = 0.f;
    s.l = kSharpenUnusable;
    const float m = sharpen_max(sharpen_max(c[0], c[1]), c[2]);
    const bool usable = pixel_finite(c[0]) && pixel_finite(c[1]) && pixel_finite(c[2]) && c[0] >= 0.f && c[1] >= 0.f && c[2] >= 0.f && m <= kSharpenMaxC;
    if (usable) {
        const float d = 1.0f + m;
        s.t[0] = (c[0] / d) + 0.0f;
        s.t[1] = (c[1] / d) + 0.0f;
        s.t[2] = (c[2] / d) + 0.0f;
        s.l = (0.2126f * s.t[0] + 0.7152f * s.t[1]) + 0.0722f * s.t[2];
    }
    return s;
}

// Step 2: what pixel E reads at a tap's place.
FF_PIXEL_HD SharpenCell sharpen_tap(const SharpenCell& E, const SharpenCell& Y) { return Y.l == kSharpenOutside ? E : Y; }

FF_PIXEL_HD bool sharpen_same(const SharpenCell& E, const SharpenCell& Y) { return Y.t[0] == E.t[0] && Y.t[1] == E.t[1] && Y.t[2] == E.t[2]; }

// Step 3 for one channel of the four taps.
FF_PIXEL_HD float sharpen_lobe(float b, float d, float f, float h)
{
    const float mn = sharpen_min(sharpen_min(b, d), sharpen_min(f, h));
    const float mx = sharpen_max(sharpen_max(b, d), sharpen_max(f, h));
    if (mx == 0.f) return -kSharpenLimit; // (black all round: limits nothing)
    return sharpen_max(-(mn / (4.0f * mx)), (1.0f - mx) / ((4.0f * mn) - 4.0f));
}

// Steps 2 to 5 for pixel E with the cells at its four taps' places (marks and all) and its radiance: out[3].
template <bool NOISE>
FF_PIXEL_HD void sharpen_pixel(float strength, const SharpenCell& E, const SharpenCell& cB, const SharpenCell& cD, const SharpenCell& cF, const SharpenCell& cH,
                               const float* rad, float* out)
{
    out[0] = rad[0];
    out[1] = rad[1];
    out[2] = rad[2];
    const SharpenCell B = sharpen_tap(E, cB), D = sharpen_tap(E, cD), F = sharpen_tap(E, cF), H = sharpen_tap(E, cH);
    if (E.l < 0.f || B.l < 0.f || D.l < 0.f || F.l < 0.f || H.l < 0.f) return;
    if (sharpen_same(E, B) && sharpen_same(E, D) && sharpen_same(E, F) && sharpen_same(E, H)) return;
    const float lr = sharpen_lobe(B.t[0], D.t[0], F.t[0], H.t[0]);
    const float lg = sharpen_lobe(B.t[1], D.t[1], F.t[1], H.t[1]);
    const float lb = sharpen_lobe(B.t[2], D.t[2], F.t[2], H.t[2]);
    float lobe = sharpen_max(-kSharpenLimit, sharpen_min(sharpen_max(sharpen_max(lr, lg), lb), 0.0f)) * strength;
    if (NOISE) {
        const float n = (0.25f * (((B.l + D.l) + F.l) + H.l)) - E.l;
        const float hi = sharpen_max(sharpen_max(sharpen_max(sharpen_max(E.l, B.l), D.l), F.l), H.l);
        const float lo = sharpen_min(sharpen_min(sharpen_min(sharpen_min(E.l, B.l), D.l), F.l), H.l);
        const float range = hi - lo;
        if (range > 0.f) {
            const float a = sharpen_min(fabsf(n) / range, 1.0f);
            lobe = lobe * (1.0f - 0.5f * a);
        }
    }
    if (lobe == 0.f) return;
    const float den = (4.0f * lobe) + 1.0f;
    float o[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float v = ((lobe * (((B.t[k] + D.t[k]) + F.t[k]) + H.t[k])) + E.t[k]) / den;
        o[k] = sharpen_min(sharpen_max(v, 0.0f), kSharpenCap);
    }
    const float M = sharpen_max(sharpen_max(o[0], o[1]), o[2]);
    const float back = 1.0f - M;
    out[0] = o[0] / back;
    out[1] = o[1] / back;
    out[2] = o[2] / back;
}

// The kernel (ff_sharpen.hip): steps 1 to 6 in one launch.  rgb8 and radiance_out may be null and must not overlap the input.
hipError_t launch_sharpen(const SharpenArgs& a, const float* radiance, unsigned char* rgb8, float* radiance_out, hipStream_t stream);

} // namespace ff
