// ff_taa.h — host-visible launch interface of the temporal anti-aliasing resolve behind ff_taa (ff_taa.hip): motion through the
// G-buffer, history resampling (Catmull-Rom or bilinear), the YCoCg neighbourhood clamp and the blend (Karis 2014, Salvi 2016).
// The formulas are in include/firefly/ff_api.h.
#pragma once

#include <hip/hip_runtime.h>

#include "ff_internal.h"
#include "ff_temporal.h" // (TemporalGeom: the per-geometry rows are the temporal denoiser's)

namespace ff {

// Everything one call needs besides the per-pixel inputs; passed by value (kernel arguments).
struct TaaArgs {
    int width, height;
    int cur;            // history buffer this call writes (1 - cur is read)
    int has_history;    // 0: the first call after a reset (nothing is read)
    int cam_rest;       // the camera is bitwise the previous call's
    int bilinear;       // FF_TAA_BILINEAR
    int clamp;          // not FF_TAA_NO_CLAMP
    int num_geoms;
    float alpha_min, gamma;
    float ray[16];      // ff_camera_ray_matrix(camera), unjittered, column-major: the far point of a miss (kernel.cu:203)
    float inv_cur[16];  // its inverse (double on the host, rounded)
    float inv_prev[16]; // inverse(ff_camera_ray_matrix(previous camera))
    float far_clip, screen_w, screen_h; // this call's camera
    float prev_screen_w, prev_screen_h; // the previous call's
    const TemporalGeom* geoms;          // per caller geometry index (kTpMoved, kTpReplaced in n[0].w)
    float4* hist[2];    // per pixel {rgb, len}
    float2* motion;     // per pixel m
};

// One launch: 16x16-pixel workgroups, the 18x18 tile of radiance with its apron in LDS.  radiance must not alias radiance_out;
// rgb8 and radiance_out may be null.
hipError_t launch_taa(const TaaArgs& a, const float* radiance, const float* position, const int* ids, unsigned char* rgb8, float* radiance_out,
                      hipStream_t stream);
// The last call's motion (W*H*2 floats) and length (W*H floats, hist[cur].w); either may be null.
hipError_t launch_taa_history(const TaaArgs& a, float* motion, float* length, hipStream_t stream);

} // namespace ff
