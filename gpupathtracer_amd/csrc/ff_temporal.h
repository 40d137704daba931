// ff_temporal.h — host-visible launch interface of the temporal denoiser behind ff_denoise_temporal (ff_temporal.hip):
// reprojection and accumulation of the history, the variance estimate and the variance-guided à-trous passes (SVGF,
// Schied et al. 2017).  The formulas are in include/firefly/ff_api.h.
#pragma once

#include <hip/hip_runtime.h>

#include "ff_internal.h"

namespace ff {

// One row of the per-geometry table, indexed by the caller's geometry index: the rigid map from this call's world to the
// previous call's, x^ = A x (A: three float4 rows of a 3x4 affine matrix), and the map of normals, n^ = N n (three float4
// rows of inverse(A)^T, xyz).  n[0].w holds the flags as int bits.
constexpr int kTpMoved = 1;    // the model matrix changed since the previous call: x^ = A x (else x^ = x exactly)
constexpr int kTpReplaced = 2; // ff_update_mesh replaced the mesh since the previous call: no history on it
struct TemporalGeom {
    float4 a[3];
    float4 n[3];
};
static_assert(sizeof(TemporalGeom) == 96, "96-byte geometry row");

// The working set.  History sets [2] swap by index between calls: set `cur` is written, set 1 - cur read.  Per pixel:
// guide {x, y, z, class} and {unit normal, 0} as DenoiseBuffers, demodulated colour history {rgb, 0}, moments {l, l^2, len, 0}.
// work[2]: the accumulated colour and its variance {rgb, var}, ping-ponged by the passes.  motion: (fx - x, fy - y).
struct TemporalBuffers {
    int width, height;
    float4* pos[2];
    float4* nrm[2];
    float4* col[2];
    float4* mom[2];
    float4* work[2];
    float2* motion;
};

struct TemporalReproject {
    int cur;           // history set this call writes
    int has_history;   // 0: the first call after a reset (nothing is read from set 1 - cur)
    int at_rest;       // the camera is bitwise the previous call's
    float proj[16];    // inverse(ff_camera_ray_matrix(previous camera)), column-major
    float eye[3];      // the previous camera's m_position
    float screen_w, screen_h; // ... and its m_screenWidth, m_screenHeight
    const TemporalGeom* geoms;
    int num_geoms;
    float reuse_normal, reuse_plane;
    float max_history;
    float variance_history;
    int demodulate;
    int feedback_unfiltered; // feedback_pass = -1: the accumulation is the next call's colour history
};

// Packs this call's guides into set cur, reprojects and accumulates: work[0] = {acc colour, temporal variance (len >=
// variance_history) or 0}, mom[cur], motion; col[cur] = acc where feedback_unfiltered.
hipError_t launch_temporal_reproject(const TemporalBuffers& b, const TemporalReproject& r, const float* radiance, const float* position,
                                     const float* normal, const float* albedo, const int* ids, hipStream_t stream);
// The 7x7 spatial variance of pixels with len < variance_history, into work[0].w.
hipError_t launch_temporal_variance(const TemporalBuffers& b, int cur, float variance_history, float inv_sigma_normal, float sigma_plane2,
                                    hipStream_t stream);
// Pass `pass` (step 2^pass) from work[src] into work[1 - src]; feedback (may be null) also receives the colour.
hipError_t launch_temporal_pass(const TemporalBuffers& b, int cur, int src, int pass, float sigma_luminance, float inv_sigma_normal,
                                float sigma_plane2, int same_geometry, float4* feedback, hipStream_t stream);
// The last call's motion (W*H*2 floats) and length (W*H floats, mom[cur].z); either may be null.
hipError_t launch_temporal_history(const TemporalBuffers& b, int cur, float* motion, float* length, hipStream_t stream);

} // namespace ff
