// ff_motion_blur.hip — the kernels behind ff_motion_blur: a motion-blur reconstruction filter on stored screen motion.  A translation
// unit of its own beside the other image kernels and the trace kernels, which it does not touch.  The
// operator is in include/firefly/ff_api.h and, as code, in ff_motion_blur.h, which the host twin ff_motion_blur_host compiles too.
// Steps (a) and (b) are ff_tile_filter.h's kernels under MotionBlurFilter:
//
//   pack_small_tiles_kernel<MotionBlurFilter, P>  (a) for k <= 8: P = 1, 4, 16, 32 or 64 lanes per tile
//   pack_tile_max_kernel<MotionBlurFilter>        (a) for k > 8: every thread packs its pixels' {v, l, z} into the float4 plane and
//                                keeps the largest 64-bit key (bits of |v|^2, inverted row-major index) among them; a wave-level max
//                                is two 32-bit shuffles per step.  The key is unique in the tile, so the thread that holds the
//                                winner writes T: no order of arrival matters
//   neighbour_max_kernel<MotionBlurFilter>        (b) the 3 x 3 maximum of T under the same key
//   mblur_gather_kernel          (c) one thread per pixel, 64 x 4 pixels per workgroup, a wave on 64 consecutive pixels of a row: one
//                                float4 and one colour per tap.  A pixel whose tile has ln <= 0.5 leaves before the tap loop; a wave
//                                that lies in such tiles alone (a camera at rest: every wave) never enters it and is a copy
#include "ff_motion_blur.h"

namespace ff {
namespace {

__global__ __launch_bounds__(256) void mblur_gather_kernel(const MotionBlurArgs a, const float4* __restrict__ plane, const float4* __restrict__ neighbour_max,
                                                           const float* __restrict__ radiance, unsigned char* __restrict__ rgb8,
                                                           float* __restrict__ radiance_out)
{
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    if (x >= a.grid.width || y >= a.grid.height) return;
    float v[3];
    mblur_gather(a, x, y, plane, radiance, neighbour_max[tile_of_pixel(a.grid, x, y)], v);
    store_rgb((size_t)y * (size_t)a.grid.width + (size_t)x, v, rgb8, radiance_out);
}

} // namespace

template hipError_t launch_pack_tile_max<MotionBlurFilter>(const MotionBlurArgs&, const float*, const float*, float4*, float4*, hipStream_t);
template hipError_t launch_neighbour_max<MotionBlurFilter>(const MotionBlurArgs&, const float4*, float4*, hipStream_t);

hipError_t MotionBlurFilter::launch_gather(const MotionBlurArgs& a, const float4* plane, const float4* neighbour_max, const float* radiance,
                                           unsigned char* rgb8, float* radiance_out, hipStream_t stream)
{
    return launch_gather_kernel(mblur_gather_kernel, a, stream, plane, neighbour_max, radiance, rgb8, radiance_out);
}

} // namespace ff
