// ff_denoise.h — host-visible launch interface of the image kernels beside the trace kernels (ff_denoise.hip): the G-buffer
// resolve behind ff_gbuffer and the edge-avoiding à-trous passes behind ff_denoise.
#pragma once

#include <hip/hip_runtime.h>

#include "ff_internal.h"

namespace ff {

// What the resolve reads: the stored primary hits of a whole frame (KParams::primary_hits, [3][pix_items] float4 in 8x8-tile item
// order, tiles_per_row tiles per row) and the scene records they name.  Pixels with x >= xlim or y >= ylim were not traced.
struct GbufferResolveParams {
    const float4* hits;
    unsigned pix_items;
    int tiles_per_row;
    int width, height, xlim, ylim;
    const GeomRecord* geoms;
    const TriRecord* tris;
    int num_geoms;
    long long num_tris;
    // albedo textures (ff_texture.h; tex_bind null: none bound): a bound diffuse hit's albedo is m_albedo times the texel at its position
    const TexBinding* tex_bind;
    const TexDesc* tex_desc;
    const TriUVs* uvs;
    // outputs, row-major, top row first (any may be null)
    float* depth;    // W*H
    float* position; // W*H*3
    float* normal;   // W*H*3
    float* albedo;   // W*H*3
    int* ids;        // W*H*3
};
hipError_t launch_gbuffer_resolve(const GbufferResolveParams& p, hipStream_t stream);

// The filter's working set: two 16-byte guide records per pixel, {x, y, z, class} and {unit normal, 0} (class: the geometry id of a
// filterable pixel, -1 for a pixel that is copied through), and float4 colour buffers (demodulated where asked).
struct DenoiseBuffers {
    int width, height;
    float4* guide_pos;
    float4* guide_nrm;
    float4* color[2];
};
// Packs the guides and the (demodulated) colour into color[0].
hipError_t launch_denoise_pack(const DenoiseBuffers& b, const float* radiance, const float* position, const float* normal, const float* albedo,
                               const int* ids, int demodulate, hipStream_t stream);
// Pass `pass` (step 2^pass) from color[src] into color[1 - src].
hipError_t launch_denoise_pass(const DenoiseBuffers& b, int src, int pass, float inv_sigma_color2, float inv_sigma_normal, float sigma_plane2,
                               int same_geometry, hipStream_t stream);
// Output: filterable pixels from color[src] (remodulated), every other pixel radiance_in bit for bit; rgb8 / radiance_out may be null
// and radiance_out may be radiance_in.  src < 0: no pass ran, every pixel is copied through.
hipError_t launch_denoise_finish(const DenoiseBuffers& b, int src, const float* radiance_in, const float* albedo, int demodulate,
                                 unsigned char* rgb8, float* radiance_out, hipStream_t stream);

} // namespace ff
