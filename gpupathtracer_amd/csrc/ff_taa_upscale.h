// ff_taa_upscale.h — host-visible launch interface of the temporal upsampler behind ff_taa_upscale (ff_taa_upscale.hip): ff_taa
// writing a larger image than it reads.  A jittered w x h frame is accumulated into a W x H history: every high pixel takes the low
// sample nearest to it with a confidence that falls off with the distance between its own ray and the ray the low pixel traced
// (a tent one high pixel wide), so a sequence of jittered low frames converges to the full-resolution image.  The formulas are in
// include/firefly/ff_api.h.
//
// Not offered: guides other than ids (normals, albedo demodulation), ff_denoise_temporal's moments at high resolution, a jittered
// high G-buffer, a multi-GPU twin.
#pragma once

#include <hip/hip_runtime.h>

#include "ff_taa.h"

namespace ff {

// Everything one call needs besides the per-pixel inputs; passed by value (kernel arguments).
struct TaaUpscaleArgs {
    TaaArgs taa;              // the W x H grid: motion, history (ff_taa's layout, so launch_taa_history reads it back), clamp, blend
    int lo_width, lo_height;  // w, h
    float lo_jx, lo_jy;       // the jitter the low frame and ids_lo were made under
    float sx, sy;             // (float)W / (float)w, (float)H / (float)h
};

// One launch: 16x16 high pixels per workgroup, the low footprint of the tile (radiance and ids) in LDS.  rgb8 and radiance_out may be
// null and must not overlap an input.
hipError_t launch_taa_upscale(const TaaUpscaleArgs& a, const float* radiance_lo, const int* ids_lo, const float* position, const int* ids,
                              unsigned char* rgb8, float* radiance_out, hipStream_t stream);

} // namespace ff
