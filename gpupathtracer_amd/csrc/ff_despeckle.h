// ff_despeckle.h — the firefly clamp behind ff_despeckle: a W x H radiance image and ff_gbuffer's albedo and ids planes give the image
// in which every pixel far brighter than its neighbours on the same surface is scaled down to a multiple of their rank-th largest
// luminance.  A windowed order statistic: a selection, no sum, so nothing depends on an order.  The per-pixel functions of steps 1,
// 2 and 3 are inline and compiled for the host and the device alike: the kernel (ff_despeckle.hip) and the host twin
// ff_despeckle_host (ff_despeckle_api.cpp) call the same code.  The operator is spelled out in include/firefly/ff_api.h.
//
// Arithmetic: float32 throughout, every expression evaluated as parenthesised below, no fused multiply-add (the library is built
// with -ffp-contract=off), true divisions (correctly rounded on the device under the library's flags).  exp, pow and sqrt appear
// nowhere, so the two sides agree bit for bit.
//
// Not offered: a temporal test against ff_denoise_temporal's moments, redistribution of the removed energy, a multi-GPU twin.
#pragma once

#include "../../include/firefly/ff_types.h"
#include <string.h>

#include "ff_pixel.h"

namespace ff {

constexpr int kDespeckleMaxRadius = 3;
constexpr int kDespeckleMaxRank = 4;
// The count of clamped pixels leaves the kernel in kDespeckleSlots partial counts (a power of two), kDespeckleSlotStride uint32
// (128 bytes) apart; a workgroup adds to the slot of its index modulo their number.
constexpr int kDespeckleSlots = 256;
constexpr int kDespeckleSlotStride = 32;

// Everything one call needs besides its buffers; passed by value (kernel arguments).  Images are row-major, top row first.
struct DespeckleArgs {
    int width, height;
    int radius, rank; // (the kernel has them as template arguments)
    int min_neighbours;
    float threshold, floor;
    int demodulate;   // FF_DESPECKLE_DEMODULATE_ALBEDO
};

// Step 1's result for one pixel: its luminance and the geometry it lies on, -1 for a pixel that does not count.
struct DespeckleCell {
    float l;
    int32_t g;
};

// Step 1's luminance of three radiance floats under three albedo floats (null without demodulation).
FF_PIXEL_HD float despeckle_luminance(const float* rad, const float* alb)
{
    float cr = rad[0], cg = rad[1], cb = rad[2];
    if (alb) {
        const float ar = alb[0], ag = alb[1], ab = alb[2];
        if (ar > 0.f) cr = cr / ar;
        if (ag > 0.f) cg = cg / ag;
        if (ab > 0.f) cb = cb / ab;
    }
    return (0.2126f * cr + 0.7152f * cg) + 0.0722f * cb;
}

// Step 1 for the pixel whose three radiance floats, three albedo floats (null without demodulation) and three ids are given.
FF_PIXEL_HD DespeckleCell despeckle_measure(const float* rad, const float* alb, const int32_t* ids)
{
    bool ok = ids[0] >= 0 && ids[2] != FF_BXDF_EMITTER && pixel_finite(rad[0]) && pixel_finite(rad[1]) && pixel_finite(rad[2]);
    if (alb) ok = ok && alb[0] == alb[0] && alb[1] == alb[1] && alb[2] == alb[2]; // (a NaN albedo spoils its pixel)
    const float l = despeckle_luminance(rad, alb);
    ok = ok && pixel_finite(l);
    DespeckleCell c;
    c.l = l;
    c.g = ok ? ids[0] : -1;
    return c;
}

// Step 2's running state for one pixel: the RANK largest luminances met so far, largest first, and the number of neighbours.  A
// list of constants' length that every loop over it unrolls: registers, no indexed memory.
template <int RANK>
struct DespeckleTop {
    float t[RANK];
    int n;
};

template <int RANK>
FF_PIXEL_HD void despeckle_begin(DespeckleTop<RANK>& s)
{
#pragma unroll
    for (int k = 0; k < RANK; ++k) s.t[k] = -INFINITY;
    s.n = 0;
}

// Window pixel Y (not X itself) of counting pixel X: a neighbour when it lies on X's geometry (a pixel that does not count has
// g = -1 and X has g >= 0).  Its luminance is finite; what is no neighbour enters as -Inf, which moves nothing.
template <int RANK>
FF_PIXEL_HD void despeckle_take(DespeckleTop<RANK>& s, const DespeckleCell& X, const DespeckleCell& Y)
{
    const bool same = Y.g == X.g;
    float v = same ? Y.l : -INFINITY;
    s.n += same ? 1 : 0;
#pragma unroll
    for (int k = 0; k < RANK; ++k) {
        const float hi = v > s.t[k] ? v : s.t[k];
        v = v > s.t[k] ? s.t[k] : v;
        s.t[k] = hi;
    }
}

constexpr int kDespeckleSteps = 64; // how often step 3 lowers its factor by one float32 before it gives the pixel up

// The float32 next below f > 0 (towards 0).
FF_PIXEL_HD float despeckle_below(float f)
{
    uint32_t u;
    memcpy(&u, &f, sizeof u);
    u -= 1u;
    memcpy(&f, &u, sizeof f);
    return f;
}

// Step 3 for counting or other pixel X with its window's state and its albedo (null without demodulation): out[3], and whether
// the pixel was clamped.  The factor limit / l is lowered one float32 at a time until the luminance of the OUTPUT, measured as
// step 1 measures, is not above the limit: the quotient, the three products and the measure are each rounded, and any of them may
// round up.  (One or two steps on real frames; radiance of mixed sign whose channels cancel can need more than the bound, and is
// then scaled by 0.)
template <int RANK>
FF_PIXEL_HD bool despeckle_clamp(const DespeckleArgs& a, const DespeckleCell& X, const DespeckleTop<RANK>& s, const float* rad, const float* alb, float* out)
{
    out[0] = rad[0];
    out[1] = rad[1];
    out[2] = rad[2];
    if (X.g < 0 || s.n < a.min_neighbours) return false;
    const float scaled = a.threshold * s.t[RANK - 1];
    const float limit = scaled > a.floor ? scaled : a.floor; // (a zero of either sign gives floor's own)
    if (!(X.l > 0.f && X.l > limit)) return false;
    float f = limit / X.l;
    for (int step = 0;; ++step) {
        out[0] = rad[0] * f;
        out[1] = rad[1] * f;
        out[2] = rad[2] * f;
        if (!(despeckle_luminance(out, alb) > limit) || !(f > 0.f)) break;
        f = step < kDespeckleSteps ? despeckle_below(f) : 0.f;
    }
    return true;
}

// The kernel (ff_despeckle.hip): steps 1 to 4 in one launch; clamped (device, kDespeckleSlots * kDespeckleSlotStride uint32, zeroed
// by the caller) receives the partial counts.  rgb8 and radiance_out may be null and must not overlap an input.
hipError_t launch_despeckle(const DespeckleArgs& a, const float* radiance, const float* albedo, const int32_t* ids, unsigned char* rgb8, float* radiance_out,
                            uint32_t* clamped, hipStream_t stream);

} // namespace ff
