// ff_display.h — host-visible launch interface of the display transform behind ff_display (ff_display.hip): luminance histogram,
// bloom pyramid, exposure, tone curve and 8-bit encoding.  The formulas are in include/firefly/ff_api.h; the per-channel curve and
// the two encodings are written once here, for the kernels and for the host twin ff_display_curve (ff_display_api.cpp).
#pragma once

#include <hip/hip_runtime.h>

#include "ff_internal.h"

namespace ff {

constexpr int kDisplayBins = 256;       // histogram bins: 8 per stop from 2^-16 up
constexpr int kDisplayThresholds = 255; // T_1 .. T_255 of FF_ENCODE_SRGB
constexpr int kDisplayMaxLevels = 8;

// Step 5 for one channel of e': x = max(e', 0) (NaN and -Inf: 0), the curve, a NaN quotient (Inf / Inf) = 1, clamp to [0, 1].
// Plain + * / only: the library is built without contraction and with IEEE division, so host and device agree bit for bit.
template <int CURVE>
__host__ __device__ __forceinline__ float display_curve(float ep, float w2)
{
    const float x = ep > 0.f ? ep : 0.f;
    float y;
    if (CURVE == FF_CURVE_REINHARD) y = (x * (1.f + x / w2)) / (1.f + x);
    else if (CURVE == FF_CURVE_ACES) y = (x * (2.51f * x + 0.03f)) / (x * (2.43f * x + 0.59f) + 0.14f);
    else y = x;
    if (y != y) y = 1.f;
    return y < 0.f ? 0.f : (y > 1.f ? 1.f : y);
}

// FF_ENCODE_LINEAR: the project's 8-bit rule (ff_k_shade.h to_u8)
__host__ __device__ __forceinline__ unsigned display_linear_u8(float y)
{
    const float s = y * 255.0f;
    if (!(s > 0.0f)) return 0;
    if (s >= 255.0f) return 255;
    return (unsigned)s;
}

// FF_ENCODE_SRGB: the number of thresholds T_1 .. T_255 (t[0 .. 254], increasing) that are <= y, in 8 steps
__host__ __device__ __forceinline__ unsigned display_srgb_u8(float y, const float* t)
{
    unsigned n = 0;
#pragma unroll
    for (unsigned step = 128; step >= 1; step >>= 1)
        if (t[n + step - 1] <= y) n += step; // (n + step <= 255)
    return n;
}

// Everything the per-pixel kernel needs besides its buffers; passed by value (kernel arguments).
struct DisplayArgs {
    int width, height;
    int curve, encoding;  // FF_CURVE_*, FF_ENCODE_*
    int bloom;            // FF_DISPLAY_BLOOM: e' = e + up(U_1) * bloom_scale
    float exposure;       // E
    float w2;             // white * white
    float bloom_scale;    // bloom_strength / bloom_levels, formed once in float
    const float* thresholds; // device copy of T_1 .. T_255
    const float4* u1;     // level 1 of the pyramid after the way up, {rgb, 0} per texel
    int u1_w, u1_h;
};

// One level of the bloom pyramid: {rgb, 0} per texel.
struct BloomLevel {
    float4* texels;
    int w, h;
};

// 256 counters (zeroed by the caller) += the histogram of radiance (W*H*3 floats), step 1 of ff_api.h.
hipError_t launch_display_histogram(const float* radiance, size_t pixels, unsigned* counters, int num_cus, hipStream_t stream);
// Level 1 = the 2x2 reduction of the bright pass of radiance * E (B_0 is never written).
hipError_t launch_bloom_bright_down(const float* radiance, int width, int height, float exposure, float threshold, BloomLevel dst, hipStream_t stream);
// dst = the 2x2 reduction of src.
hipError_t launch_bloom_down(BloomLevel src, BloomLevel dst, hipStream_t stream);
// dst += up(src), in place (U_j = D_j + up(U_{j+1})).
hipError_t launch_bloom_up(BloomLevel src, BloomLevel dst, hipStream_t stream);
// Steps 3 to 6.  rgb8 and display_out may be null; display_out may be radiance itself.
hipError_t launch_display(const DisplayArgs& a, const float* radiance, unsigned char* rgb8, float* display_out, hipStream_t stream);

} // namespace ff
