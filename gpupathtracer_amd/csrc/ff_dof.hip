// ff_dof.hip — the kernels behind ff_depth_of_field: a gather depth-of-field filter on the G-buffer.  A translation unit of its own
// beside the other image kernels and the trace kernels, which it does not touch.  The operator is in
// include/firefly/ff_api.h and, as code, in ff_dof.h, which the host twin ff_depth_of_field_host compiles too.  Steps (a) and (b)
// are ff_tile_filter.h's kernels under DofFilter:
//
//   pack_small_tiles_kernel<DofFilter, P>  (a) for k <= 8: P = 1, 4, 16, 32 or 64 lanes per tile; the group's first lane writes T
//   pack_tile_max_kernel<DofFilter>        (a) for k > 8: every thread packs its pixels' {l, zk} into the float2 plane and keeps the
//                               largest l among them; a wave-level max is six shuffles.  l is finite and >= 0: a plain float
//                               maximum that can tie, so thread 0 alone combines the waves and writes T
//   neighbour_max_kernel<DofFilter>        (b) the 3 x 3 maximum of T
//   dof_gather_kernel           (c) one thread per pixel, 64 x 4 pixels per workgroup, a wave on 64 consecutive pixels of a row: one
//                               float2 and one colour per tap.  A pixel whose tile has n <= 0.5 leaves before the tap loop; a wave
//                               that lies in such tiles alone (everything in focus: every wave) never enters it and is a copy.
//                               The tap grid's column offsets are formed once per pixel into a column of bytes in LDS that the
//                               thread alone reads back (no barrier)
#include "ff_dof.h"

namespace ff {
namespace {

constexpr int kGatherThreads = 256;

__global__ __launch_bounds__(kGatherThreads) void dof_gather_kernel(const DofArgs a, const float2* __restrict__ plane, const float* __restrict__ neighbour_max,
                                                                    const float* __restrict__ radiance, unsigned char* __restrict__ rgb8,
                                                                    float* __restrict__ radiance_out)
{
    // the column offsets of the tap grid, one column of 2g + 1 bytes per thread: entry i of thread t at s_dx[i * 256 + t]
    __shared__ signed char s_dx[kDofColumns * kGatherThreads];
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    if (x >= a.grid.width || y >= a.grid.height) return;
    float v[3];
    dof_gather(a, x, y, plane, radiance, neighbour_max[tile_of_pixel(a.grid, x, y)], s_dx + (threadIdx.y * 64 + threadIdx.x), kGatherThreads, v);
    store_rgb((size_t)y * (size_t)a.grid.width + (size_t)x, v, rgb8, radiance_out);
}

} // namespace

template hipError_t launch_pack_tile_max<DofFilter>(const DofArgs&, const float*, const float*, float2*, float*, hipStream_t);
template hipError_t launch_neighbour_max<DofFilter>(const DofArgs&, const float*, float*, hipStream_t);

hipError_t DofFilter::launch_gather(const DofArgs& a, const float2* plane, const float* neighbour_max, const float* radiance, unsigned char* rgb8,
                                    float* radiance_out, hipStream_t stream)
{
    return launch_gather_kernel(dof_gather_kernel, a, stream, plane, neighbour_max, radiance, rgb8, radiance_out);
}

} // namespace ff
