// ff_motion_blur.hip — the kernels behind ff_motion_blur: a motion-blur reconstruction filter on stored screen motion.  A translation
// unit of its own beside the other image kernels and the trace kernels, which it does not touch.  The
// operator is in include/firefly/ff_api.h and, as code, in ff_motion_blur.h, which the host twin ff_motion_blur_host compiles too.
//
//   mblur_pack_small_tiles_kernel (a) for k <= 8: 1, 4, 16, 32 or 64 lanes per tile, 256 / that many tiles per workgroup, the keys
//                                meet in shuffles inside the lane group
//   mblur_pack_tile_max_kernel   (a) for k > 8, one workgroup of 256 threads per k x k tile: every thread packs its pixels' {v, l, z}
//                                into the float4 plane and keeps the largest 64-bit key (bits of |v|^2, inverted row-major index) among them; the keys meet in
//                                a wave-level max (two 32-bit shuffles per step), then across the waves through LDS.  The key is
//                                unique in the tile, so the thread that holds the winner writes T: no order of arrival matters
//   mblur_neighbour_max_kernel   (b) one thread per tile: the 3 x 3 maximum of T under the same key
//   mblur_gather_kernel          (c) one thread per pixel, 64 x 4 pixels per workgroup, a wave on 64 consecutive pixels of a row: one
//                                float4 and one colour per tap.  A pixel whose tile has ln <= 0.5 leaves before the tap loop; a wave
//                                that lies in such tiles alone (a camera at rest: every wave) never enters it and is a copy
//
// Every output is a function of its own inputs alone: nothing depends on the order of floating-point adds or of the workgroups.
#include "ff_motion_blur.h"

namespace ff {
namespace {

constexpr int kTileThreads = 256;

__global__ __launch_bounds__(kTileThreads) void mblur_pack_tile_max_kernel(const MotionBlurArgs a, const float* __restrict__ motion,
                                                                           const float* __restrict__ depth, float4* __restrict__ plane,
                                                                           float4* __restrict__ tile_max)
{
    __shared__ unsigned long long s_key[kTileThreads / 64];
    const int x0 = blockIdx.x * a.k, y0 = blockIdx.y * a.k;
    const int tw = min(a.k, a.width - x0), th = min(a.k, a.height - y0); // (partial tiles at the right and bottom edges)
    const int count = tw * th;
    unsigned long long best = 0; // (every pixel's key is above 0: its low word is at least 2^32 - 4096)
    float4 best_p = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int i = threadIdx.x; i < count; i += blockDim.x) {
        const int ly = i / tw, lx = i - ly * tw; // i is the pixel's row-major index in the tile
        const size_t p = (size_t)(y0 + ly) * (size_t)a.width + (size_t)(x0 + lx);
        const float4 v = mblur_pack(a, motion[2 * p], motion[2 * p + 1], depth[p]);
        plane[p] = v;
        const unsigned long long key = mblur_key(v.x, v.y, (unsigned)i);
        if (key > best) {
            best = key;
            best_p = v;
        }
    }
    unsigned long long win = best;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const unsigned long long other = __shfl_xor(win, off, 64);
        win = other > win ? other : win;
    }
    const int waves = blockDim.x >> 6;
    if ((threadIdx.x & 63) == 0) s_key[threadIdx.x >> 6] = win;
    __syncthreads();
    for (int w = 0; w < waves; ++w) win = s_key[w] > win ? s_key[w] : win;
    if (best == win) tile_max[(size_t)blockIdx.y * (size_t)a.tiles_x + (size_t)blockIdx.x] = make_float4(best_p.x, best_p.y, best_p.z, 0.f);
}

// (a) for tiles of at most 64 pixels (k <= 8): a group of P = GROUP consecutive lanes per tile, P the power of two that holds k * k,
// 256 / P tiles per workgroup in row-major order of the tiles.  Lane i of a group packs the tile's pixel i; the keys meet in log2 P
// shuffle steps that stay inside the group, and the lane that holds the winner writes T.  No LDS, no idle waves: at k = 1 a lane
// is a tile and consecutive lanes are consecutive pixels.
template <int GROUP>
__global__ __launch_bounds__(kTileThreads) void mblur_pack_small_tiles_kernel(const MotionBlurArgs a, const float* __restrict__ motion,
                                                                              const float* __restrict__ depth, float4* __restrict__ plane,
                                                                              float4* __restrict__ tile_max)
{
    const size_t tiles = (size_t)a.tiles_x * (size_t)a.tiles_y;
    const size_t tile = (size_t)blockIdx.x * (kTileThreads / GROUP) + threadIdx.x / GROUP;
    const int i = threadIdx.x % GROUP;
    unsigned long long best = 0; // (a lane without a pixel: below every pixel's key)
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (tile < tiles) {
        const int x0 = (int)(tile % (size_t)a.tiles_x) * a.k, y0 = (int)(tile / (size_t)a.tiles_x) * a.k;
        const int tw = min(a.k, a.width - x0), th = min(a.k, a.height - y0);
        if (i < tw * th) {
            const int ly = i / tw, lx = i - ly * tw;
            const size_t p = (size_t)(y0 + ly) * (size_t)a.width + (size_t)(x0 + lx);
            v = mblur_pack(a, motion[2 * p], motion[2 * p + 1], depth[p]);
            plane[p] = v;
            best = mblur_key(v.x, v.y, (unsigned)i);
        }
    }
    unsigned long long win = best;
#pragma unroll
    for (int off = GROUP / 2; off >= 1; off >>= 1) {
        const unsigned long long other = __shfl_xor(win, off, 64);
        win = other > win ? other : win;
    }
    if (best != 0 && best == win) tile_max[tile] = make_float4(v.x, v.y, v.z, 0.f);
}

template <int GROUP>
void launch_small_tiles(const MotionBlurArgs& a, const float* motion, const float* depth, float4* plane, float4* tile_max, hipStream_t stream)
{
    const size_t tiles = (size_t)a.tiles_x * (size_t)a.tiles_y, per_block = kTileThreads / GROUP;
    hipLaunchKernelGGL(mblur_pack_small_tiles_kernel<GROUP>, dim3((unsigned)((tiles + per_block - 1) / per_block)), dim3(kTileThreads), 0, stream, a, motion,
                       depth, plane, tile_max);
}

__global__ __launch_bounds__(256) void mblur_neighbour_max_kernel(const MotionBlurArgs a, const float4* __restrict__ tile_max,
                                                                  float4* __restrict__ neighbour_max)
{
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= (size_t)a.tiles_x * (size_t)a.tiles_y) return;
    neighbour_max[t] = mblur_neighbour_max(a, tile_max, (int)(t % (size_t)a.tiles_x), (int)(t / (size_t)a.tiles_x));
}

__global__ __launch_bounds__(256) void mblur_gather_kernel(const MotionBlurArgs a, const float4* __restrict__ plane, const float4* __restrict__ neighbour_max,
                                                           const float* __restrict__ radiance, unsigned char* __restrict__ rgb8,
                                                           float* __restrict__ radiance_out)
{
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    if (x >= a.width || y >= a.height) return;
    const size_t i = (size_t)y * (size_t)a.width + (size_t)x;
    const float4 n = neighbour_max[(size_t)(y / a.k) * (size_t)a.tiles_x + (size_t)(x / a.k)];
    float v[3];
    mblur_gather(a, x, y, plane, radiance, n, v);
    if (radiance_out) { radiance_out[3 * i] = v[0]; radiance_out[3 * i + 1] = v[1]; radiance_out[3 * i + 2] = v[2]; }
    if (rgb8) { rgb8[3 * i] = mblur_u8(v[0]); rgb8[3 * i + 1] = mblur_u8(v[1]); rgb8[3 * i + 2] = mblur_u8(v[2]); }
}

} // namespace

hipError_t launch_mblur_pack_tile_max(const MotionBlurArgs& a, const float* motion, const float* depth, float4* plane, float4* tile_max, hipStream_t stream)
{
    if (a.width <= 0 || a.height <= 0) return hipSuccess;
    // a tile of at most 64 pixels is the work of a part of a wave: several tiles per workgroup
    const int pixels = a.k * a.k;
    if (pixels <= 1) launch_small_tiles<1>(a, motion, depth, plane, tile_max, stream);
    else if (pixels <= 4) launch_small_tiles<4>(a, motion, depth, plane, tile_max, stream);
    else if (pixels <= 16) launch_small_tiles<16>(a, motion, depth, plane, tile_max, stream);
    else if (pixels <= 32) launch_small_tiles<32>(a, motion, depth, plane, tile_max, stream);
    else if (pixels <= 64) launch_small_tiles<64>(a, motion, depth, plane, tile_max, stream);
    else hipLaunchKernelGGL(mblur_pack_tile_max_kernel, dim3((unsigned)a.tiles_x, (unsigned)a.tiles_y), dim3(kTileThreads), 0, stream, a, motion, depth, plane, tile_max);
    return hipGetLastError();
}

hipError_t launch_mblur_neighbour_max(const MotionBlurArgs& a, const float4* tile_max, float4* neighbour_max, hipStream_t stream)
{
    const size_t tiles = (size_t)a.tiles_x * (size_t)a.tiles_y;
    if (tiles == 0) return hipSuccess;
    hipLaunchKernelGGL(mblur_neighbour_max_kernel, dim3((unsigned)((tiles + 255) / 256)), dim3(256), 0, stream, a, tile_max, neighbour_max);
    return hipGetLastError();
}

hipError_t launch_mblur_gather(const MotionBlurArgs& a, const float4* plane, const float4* neighbour_max, const float* radiance, unsigned char* rgb8,
                               float* radiance_out, hipStream_t stream)
{
    if (a.width <= 0 || a.height <= 0) return hipSuccess;
    const dim3 grid((unsigned)((a.width + 63) / 64), (unsigned)((a.height + 3) / 4));
    hipLaunchKernelGGL(mblur_gather_kernel, grid, dim3(64, 4), 0, stream, a, plane, neighbour_max, radiance, rgb8, radiance_out);
    return hipGetLastError();
}

} // namespace ff
