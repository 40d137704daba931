// ff_adaptive.hip — the kernels behind ff_render_adaptive.  A translation unit of its own beside the image kernels and the trace
// kernels, which it does not touch.  The estimator is in include/firefly/ff_api.h and, as code, in
// ff_adaptive.h, which the host twin ff_adaptive_tile_error_host compiles too.
//
//   adaptive_accumulate_kernel   one thread per float of a compact w x h x 3 rectangle: a wave reads 256 consecutive bytes of the
//                                work buffer and adds them to the two sum planes at (x0, y0).  Pass 0 writes instead of adding
//                                (ff_render_progressive's first frame does the same), so a call needs no clear of the planes.
//   adaptive_tile_error_kernel   one workgroup of 256 threads per listed tile.  Lane j adds e_j, e_(j+256), ... of the tile's
//                                row-major pixels from 0.0f (ff_adaptive.h adaptive_lane_sum); the 256 partial sums meet in LDS in
//                                the halving tree v[j] += v[j + off], off = 128 .. 1, a barrier per step; thread 0 scales and
//                                stores E_t.  The order is the definition's, whatever the grid.
//   adaptive_resolve_kernel      one thread per pixel: the mean over the pixel's tile's passes, the rgb8 of it, and the pass count.
#include "ff_adaptive.h"

namespace ff {
namespace {

constexpr int kThreads = kAdaptiveLanes;

__global__ __launch_bounds__(kThreads) void adaptive_accumulate_kernel(float* __restrict__ sum, float* __restrict__ sum_even, const float* __restrict__ work,
                                                                       int width, int x0, int y0, int w, int h, int first, int even)
{
    const size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x;
    const size_t row_floats = (size_t)w * 3;
    if (i >= row_floats * (size_t)h) return;
    const size_t row = i / row_floats, col = i - row * row_floats;
    const size_t dst = (((size_t)y0 + row) * (size_t)width + (size_t)x0) * 3 + col;
    const float v = work[i];
    sum[dst] = first ? v : sum[dst] + v;
    if (even) sum_even[dst] = first ? v : sum_even[dst] + v;
}

__global__ __launch_bounds__(kThreads) void adaptive_tile_error_kernel(const AdaptiveArgs a, const float* __restrict__ sum, const float* __restrict__ sum_even,
                                                                       const uint32_t* __restrict__ tiles, float* __restrict__ tile_error)
{
    __shared__ float s_v[kThreads];
    const uint32_t tile = tiles ? tiles[blockIdx.x] : blockIdx.x;
    const int tx = (int)(tile % (uint32_t)a.grid.tiles_x), ty = (int)(tile / (uint32_t)a.grid.tiles_x);
    s_v[threadIdx.x] = adaptive_lane_sum(a, tx, ty, (int)threadIdx.x, sum, sum_even);
    __syncthreads();
#pragma unroll
    for (int off = kThreads / 2; off >= 1; off >>= 1) {
        if ((int)threadIdx.x < off) s_v[threadIdx.x] = s_v[threadIdx.x] + s_v[threadIdx.x + off];
        __syncthreads();
    }
    if (threadIdx.x == 0) tile_error[tile] = adaptive_tile_scale(a, s_v[0], adaptive_tile_pixels(a.grid, tx, ty));
}

__global__ __launch_bounds__(kThreads) void adaptive_resolve_kernel(const TileGrid grid, const float* __restrict__ sum, const uint16_t* __restrict__ tile_passes,
                                                                    float* __restrict__ radiance, unsigned char* __restrict__ rgb8, uint16_t* __restrict__ passes)
{
    const int x = (int)(blockIdx.x * 64 + threadIdx.x), y = (int)(blockIdx.y * 4 + threadIdx.y);
    if (x >= grid.width || y >= grid.height) return;
    const size_t p = (size_t)y * (size_t)grid.width + (size_t)x;
    const uint16_t n_t = tile_passes[tile_of_pixel(grid, x, y)];
    const float inv = 1.0f / (float)n_t;
    const float v[3] = { sum[3 * p] * inv, sum[3 * p + 1] * inv, sum[3 * p + 2] * inv };
    store_rgb(p, v, rgb8, radiance);
    if (passes) passes[p] = n_t;
}

} // namespace

hipError_t launch_adaptive_accumulate(float* sum, float* sum_even, const float* work, int width, int x0, int y0, int w, int h, int first, int even,
                                      hipStream_t stream)
{
    if (w <= 0 || h <= 0) return hipSuccess;
    const size_t values = (size_t)w * (size_t)h * 3;
    hipLaunchKernelGGL(adaptive_accumulate_kernel, dim3((unsigned)((values + kThreads - 1) / kThreads)), dim3(kThreads), 0, stream, sum, sum_even, work, width,
                       x0, y0, w, h, first, even);
    return hipGetLastError();
}

hipError_t launch_adaptive_tile_error(const AdaptiveArgs& a, const float* sum, const float* sum_even, const uint32_t* tiles, int count, float* tile_error,
                                      hipStream_t stream)
{
    if (count <= 0) return hipSuccess;
    hipLaunchKernelGGL(adaptive_tile_error_kernel, dim3((unsigned)count), dim3(kThreads), 0, stream, a, sum, sum_even, tiles, tile_error);
    return hipGetLastError();
}

hipError_t launch_adaptive_resolve(const TileGrid& grid, const float* sum, const uint16_t* tile_passes, float* radiance, unsigned char* rgb8, uint16_t* passes,
                                   hipStream_t stream)
{
    if (grid.width <= 0 || grid.height <= 0) return hipSuccess;
    hipLaunchKernelGGL(adaptive_resolve_kernel, dim3((unsigned)((grid.width + 63) / 64), (unsigned)((grid.height + 3) / 4)), dim3(64, 4), 0, stream, grid, sum,
                       tile_passes, radiance, rgb8, passes);
    return hipGetLastError();
}

} // namespace ff
