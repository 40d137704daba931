// ff_resize.h — the separable polyphase resampling behind ff_resize: a W x H radiance image gives a W' x H' one, each size within a
// factor of 16 of the other, under a box, triangle, Mitchell-Netravali or Lanczos-3 filter that is stretched when it minifies.  Two
// passes, the horizontal one first (W x H -> W' x H), each a weighted sum over a per-axis table of T taps per output sample that
// the host computes in double (ff_resize_api.cpp).  The per-tap functions are inline and compiled for the host and the device alike:
// the kernels (ff_resize.hip) and the host twin ff_resize_host (ff_resize_api.cpp) call the same code.  The operator is spelled out
// in include/firefly/ff_api.h.
//
// Arithmetic: float32 throughout, acc = acc + w * v with the product rounded before the sum (the library is built with
// -ffp-contract=off), min and max as written below; nothing else, so the two sides agree bit for bit.
//
// Not offered: other channel counts, a G-buffer-aware form, gamma-space resampling, a row pitch, a multi-GPU twin, a resize fused
// into ff_encode_yuv.
#pragma once

#include "../../include/firefly/ff_types.h"

#include "ff_pixel.h"

namespace ff {

constexpr int kResizeMaxRatio = 16; // out <= 16 in and in <= 16 out per axis
constexpr int kResizeMaxTaps = 96;  // T at LANCZOS3, 16 : 1

// The kernels' tiles (ff_resize.hip): the horizontal pass works on 64 output columns of kResizeRowsH rows of the input - of
// kResizeRowsHSmall where the staged input span and the weights of the larger tile would not fit kResizeLdsBytes of LDS -, the
// vertical pass on 64 output columns of 16 output rows.
constexpr int kResizeTileX = 64;
constexpr int kResizeRowsH = 4, kResizeRowsHSmall = 2;
constexpr int kResizeRowsV = 16;
constexpr size_t kResizeLdsBytes = 65536;

// One axis' table on the device.  `first` holds out_size entries.  `weights` holds out_size * taps floats: tap-major
// (weights[j * out_size + X]) for the horizontal pass, whose lanes are neighbouring outputs, and output-major
// (weights[Y * taps + j], ff_resize_weights' layout) for the vertical pass, whose waves share one output row.
struct ResizeAxis {
    const int32_t* first;
    const float* weights;
    int in_size, out_size, taps;
    int span; // horizontal pass: the most input samples a tile of kResizeTileX outputs names (after the clamp)
};

// Everything one call needs besides its buffers; passed by value (kernel arguments).  Images are row-major, top row first.
struct ResizeArgs {
    ResizeAxis x, y;
    int anti_ring; // FF_RESIZE_ANTI_RING (the kernels have it as a template argument)
    int rows_h;    // rows per tile of the horizontal pass: kResizeRowsH or kResizeRowsHSmall
};

// min and max as the header defines them (a NaN never reaches them).
FF_PIXEL_HD float resize_min(float a, float b) { return b < a ? b : a; }
FF_PIXEL_HD float resize_max(float a, float b) { return a < b ? b : a; }

// What a tap reads: a non-finite sample reads as +0.
FF_PIXEL_HD float resize_value(float v) { return pixel_finite(v) ? v : 0.f; }

// The input index of tap j of an output whose first tap is `first`, on an axis of n samples.
FF_PIXEL_HD int resize_index(int first, int j, int n)
{
    const int i = first + j;
    return i < 0 ? 0 : (i > n - 1 ? n - 1 : i);
}

// One channel of one output sample: begin, one tap after the other (v already through resize_value), finish.  lo and hi start
// outside every finite value, so the first tap with a weight sets them; an output always has one (the largest weight of a row
// is at least 1 / T).
struct ResizeSum {
    float acc, lo, hi;
};

FF_PIXEL_HD ResizeSum resize_begin()
{
    ResizeSum s;
    s.acc = 0.f;
    s.lo = INFINITY;
    s.hi = -INFINITY;
    return s;
}

template <bool RING>
FF_PIXEL_HD void resize_tap(ResizeSum& s, float w, float v)
{
    s.acc = s.acc + w * v;
    if (RING && w != 0.f) {
        s.lo = resize_min(s.lo, v);
        s.hi = resize_max(s.hi, v);
    }
}

template <bool RING>
FF_PIXEL_HD float resize_finish(const ResizeSum& s)
{
    return RING ? resize_min(resize_max(s.acc, s.lo), s.hi) : s.acc;
}

// The kernels (ff_resize.hip): the horizontal pass radiance (x.in_size x y.in_size) -> mid (x.out_size x y.in_size), then the
// vertical pass mid -> rgb8 / radiance_out (x.out_size x y.out_size), either of which may be null.  No buffer may overlap another.
hipError_t launch_resize(const ResizeArgs& a, const float* radiance, float* mid, unsigned char* rgb8, float* radiance_out, hipStream_t stream);

// The LDS bytes a tile of `rows` rows of the horizontal pass takes: the staged spans, then the weights of its kResizeTileX outputs.
inline size_t resize_lds_bytes(int rows, int span, int taps) { return ((size_t)rows * 3 * (size_t)span + (size_t)kResizeTileX * (size_t)taps) * sizeof(float); }

} // namespace ff
