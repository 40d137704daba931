// ff_dof.hip — the kernels behind ff_depth_of_field: a gather depth-of-field filter on the G-buffer.  A translation unit of its own
// beside the other image kernels and the trace kernels, which it does not touch.  The operator is in
// include/firefly/ff_api.h and, as code, in ff_dof.h, which the host twin ff_depth_of_field_host compiles too.
//
//   dof_pack_small_tiles_kernel (a) for k <= 8: 1, 4, 16, 32 or 64 lanes per tile, 256 / that many tiles per workgroup, the radii
//                               meet in shuffles inside the lane group
//   dof_pack_tile_max_kernel    (a) for k > 8, one workgroup of 256 threads per k x k tile: every thread packs its pixels' {l, zk}
//                               into the float2 plane and keeps the largest l among them; the maxima meet in a wave-level max (six
//                               shuffles), then across the waves through LDS.  l is finite and >= 0: a plain float maximum, no
//                               order of arrival matters
//   dof_neighbour_max_kernel    (b) one thread per tile: the 3 x 3 maximum of T
//   dof_gather_kernel           (c) one thread per pixel, 64 x 4 pixels per workgroup, a wave on 64 consecutive pixels of a row: one
//                               float2 and one colour per tap.  A pixel whose tile has n <= 0.5 leaves before the tap loop; a wave
//                               that lies in such tiles alone (everything in focus: every wave) never enters it and is a copy.
//                               The tap grid's column offsets are formed once per pixel into a column of bytes in LDS that the
//                               thread alone reads back (no barrier)
//
// Every output is a function of its own inputs alone: nothing depends on the order of floating-point adds or of the workgroups.
#include "ff_dof.h"

namespace ff {
namespace {

constexpr int kTileThreads = 256;
constexpr int kGatherThreads = 256;

__global__ __launch_bounds__(kTileThreads) void dof_pack_tile_max_kernel(const DofArgs a, const float* __restrict__ position,
                                                                         const float* __restrict__ depth, float2* __restrict__ plane,
                                                                         float* __restrict__ tile_max)
{
    __shared__ float s_max[kTileThreads / 64];
    const int x0 = blockIdx.x * a.k, y0 = blockIdx.y * a.k;
    const int tw = min(a.k, a.width - x0), th = min(a.k, a.height - y0); // (partial tiles at the right and bottom edges)
    const int count = tw * th;
    float best = 0.f;
    for (int i = threadIdx.x; i < count; i += kTileThreads) {
        const int ly = i / tw, lx = i - ly * tw;
        const size_t p = (size_t)(y0 + ly) * (size_t)a.width + (size_t)(x0 + lx);
        const float2 v = dof_pack(a, position[3 * p], position[3 * p + 1], position[3 * p + 2], depth[p]);
        plane[p] = v;
        best = v.x > best ? v.x : best;
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const float other = __shfl_xor(best, off, 64);
        best = other > best ? other : best;
    }
    if ((threadIdx.x & 63) == 0) s_max[threadIdx.x >> 6] = best;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < kTileThreads / 64; ++w) best = s_max[w] > best ? s_max[w] : best;
        tile_max[(size_t)blockIdx.y * (size_t)a.tiles_x + (size_t)blockIdx.x] = best;
    }
}

// (a) for tiles of at most 64 pixels (k <= 8): a group of P = GROUP consecutive lanes per tile, P the power of two that holds k * k,
// 256 / P tiles per workgroup in row-major order of the tiles.  Lane i of a group packs the tile's pixel i; the radii meet in log2 P
// shuffle steps that stay inside the group, and the group's first lane writes T.  No LDS, no idle waves: at k = 1 a lane is a tile
// and consecutive lanes are consecutive pixels.
template <int GROUP>
__global__ __launch_bounds__(kTileThreads) void dof_pack_small_tiles_kernel(const DofArgs a, const float* __restrict__ position,
                                                                            const float* __restrict__ depth, float2* __restrict__ plane,
                                                                            float* __restrict__ tile_max)
{
    const size_t tiles = (size_t)a.tiles_x * (size_t)a.tiles_y;
    const size_t tile = (size_t)blockIdx.x * (kTileThreads / GROUP) + threadIdx.x / GROUP;
    const int i = threadIdx.x % GROUP;
    float best = 0.f; // (a lane without a pixel: no radius)
    if (tile < tiles) {
        const int x0 = (int)(tile % (size_t)a.tiles_x) * a.k, y0 = (int)(tile / (size_t)a.tiles_x) * a.k;
        const int tw = min(a.k, a.width - x0), th = min(a.k, a.height - y0);
        if (i < tw * th) {
            const int ly = i / tw, lx = i - ly * tw;
            const size_t p = (size_t)(y0 + ly) * (size_t)a.width + (size_t)(x0 + lx);
            const float2 v = dof_pack(a, position[3 * p], position[3 * p + 1], position[3 * p + 2], depth[p]);
            plane[p] = v;
            best = v.x;
        }
    }
#pragma unroll
    for (int off = GROUP / 2; off >= 1; off >>= 1) {
        const float other = __shfl_xor(best, off, 64);
        best = other > best ? other : best;
    }
    if (i == 0 && tile < tiles) tile_max[tile] = best;
}

template <int GROUP>
void launch_small_tiles(const DofArgs& a, const float* position, const float* depth, float2* plane, float* tile_max, hipStream_t stream)
{
    const size_t tiles = (size_t)a.tiles_x * (size_t)a.tiles_y, per_block = kTileThreads / GROUP;
    hipLaunchKernelGGL(dof_pack_small_tiles_kernel<GROUP>, dim3((unsigned)((tiles + per_block - 1) / per_block)), dim3(kTileThreads), 0, stream, a, position,
                       depth, plane, tile_max);
}

__global__ __launch_bounds__(256) void dof_neighbour_max_kernel(const DofArgs a, const float* __restrict__ tile_max, float* __restrict__ neighbour_max)
{
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= (size_t)a.tiles_x * (size_t)a.tiles_y) return;
    neighbour_max[t] = dof_neighbour_max(a, tile_max, (int)(t % (size_t)a.tiles_x), (int)(t / (size_t)a.tiles_x));
}

__global__ __launch_bounds__(kGatherThreads) void dof_gather_kernel(const DofArgs a, const float2* __restrict__ plane, const float* __restrict__ neighbour_max,
                                                                    const float* __restrict__ radiance, unsigned char* __restrict__ rgb8,
                                                                    float* __restrict__ radiance_out)
{
    // the column offsets of the tap grid, one column of 2g + 1 bytes per thread: entry i of thread t at s_dx[i * 256 + t]
    __shared__ signed char s_dx[kDofColumns * kGatherThreads];
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    if (x >= a.width || y >= a.height) return;
    const size_t i = (size_t)y * (size_t)a.width + (size_t)x;
    const float n = neighbour_max[(size_t)(y / a.k) * (size_t)a.tiles_x + (size_t)(x / a.k)];
    float v[3];
    dof_gather(a, x, y, plane, radiance, n, s_dx + (threadIdx.y * 64 + threadIdx.x), kGatherThreads, v);
    if (radiance_out) { radiance_out[3 * i] = v[0]; radiance_out[3 * i + 1] = v[1]; radiance_out[3 * i + 2] = v[2]; }
    if (rgb8) { rgb8[3 * i] = dof_u8(v[0]); rgb8[3 * i + 1] = dof_u8(v[1]); rgb8[3 * i + 2] = dof_u8(v[2]); }
}

} // namespace

hipError_t launch_dof_pack_tile_max(const DofArgs& a, const float* position, const float* depth, float2* plane, float* tile_max, hipStream_t stream)
{
    if (a.width <= 0 || a.height <= 0) return hipSuccess;
    // a tile of at most 64 pixels is the work of a part of a wave: several tiles per workgroup
    const int pixels = a.k * a.k;
    if (pixels <= 1) launch_small_tiles<1>(a, position, depth, plane, tile_max, stream);
    else if (pixels <= 4) launch_small_tiles<4>(a, position, depth, plane, tile_max, stream);
    else if (pixels <= 16) launch_small_tiles<16>(a, position, depth, plane, tile_max, stream);
    else if (pixels <= 32) launch_small_tiles<32>(a, position, depth, plane, tile_max, stream);
    else if (pixels <= 64) launch_small_tiles<64>(a, position, depth, plane, tile_max, stream);
    else hipLaunchKernelGGL(dof_pack_tile_max_kernel, dim3((unsigned)a.tiles_x, (unsigned)a.tiles_y), dim3(kTileThreads), 0, stream, a, position, depth, plane, tile_max);
    return hipGetLastError();
}

hipError_t launch_dof_neighbour_max(const DofArgs& a, const float* tile_max, float* neighbour_max, hipStream_t stream)
{
    const size_t tiles = (size_t)a.tiles_x * (size_t)a.tiles_y;
    if (tiles == 0) return hipSuccess;
    hipLaunchKernelGGL(dof_neighbour_max_kernel, dim3((unsigned)((tiles + 255) / 256)), dim3(256), 0, stream, a, tile_max, neighbour_max);
    return hipGetLastError();
}

hipError_t launch_dof_gather(const DofArgs& a, const float2* plane, const float* neighbour_max, const float* radiance, unsigned char* rgb8,
                             float* radiance_out, hipStream_t stream)
{
    if (a.width <= 0 || a.height <= 0) return hipSuccess;
    const dim3 grid((unsigned)((a.width + 63) / 64), (unsigned)((a.height + 3) / 4));
    hipLaunchKernelGGL(dof_gather_kernel, grid, dim3(64, 4), 0, stream, a, plane, neighbour_max, radiance, rgb8, radiance_out);
    return hipGetLastError();
}

} // namespace ff
