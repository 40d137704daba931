// ff_local_tonemap.hip — the kernels behind ff_local_tonemap: bilateral-grid local tone mapping of a radiance image.  A translation
// unit of its own beside the other image kernels and the trace kernels, which it does not touch.  The
// operator is in include/firefly/ff_api.h and, as code, in ff_local_tonemap.h, which the host twins compile too.
//
//   ltm_splat_kernel<S>     steps 1 and 2.  One workgroup of 256 threads per grid column, that is per tile of S x S pixels, whose
//                           kLtmBins cells it owns: the threads stride over the tile and add count and q10 into two int arrays in
//                           LDS with LDS integer atomics (one pair of arrays per wave, as ff_display's histogram has them; a
//                           thread merges a run of pixels of one bin into one add), then the first kLtmBins threads add the waves'
//                           arrays and write the column - empty cells too, so the grid needs no clear.  No global atomics; integer
//                           adds, so the grid does not depend on their order.  S = 8: four tiles side by side (32 x 8 pixels) to a
//                           workgroup, one pair of arrays per tile.
//   ltm_blur_kernel<AXIS>   step 3, one launch per axis, a thread per cell, ping-pong between the work buffer's two grids.  The x
//                           pass reads the splat's integers and converts them.
//   ltm_slice_kernel<COPY>  steps 4 to 6: a thread per pixel over tiles of 32 x 8, the eight taps from the blurred grid (8-byte
//                           loads; the grid is small and stays in L2).  COPY: compression == 1 and detail == 1 - no grid is built,
//                           the kernel only copies (and makes rgb8).  A thread reads its own pixel before it writes it, so
//                           radiance_out may be radiance: no __restrict__ on the two.
#include "ff_local_tonemap.h"

namespace ff {
namespace {

constexpr int kThreads = 256, kWaves = kThreads / 64;
constexpr int kTileW = 32, kTileH = 8;

template <int S>
__global__ __launch_bounds__(kThreads) void ltm_splat_kernel(const LtmArgs a, const float* __restrict__ radiance, LtmCellI* __restrict__ grid)
{
    constexpr int kTiles = S == 8 ? 4 : 1;  // tiles side by side per workgroup
    constexpr int kRowW = kTiles * S;       // the workgroup's pixel rectangle: kRowW x S
    static_assert(kRowW * S % kThreads == 0, "every thread takes the same number of pixels");
    __shared__ int s_n[kWaves][kLtmBins], s_S[kWaves][kLtmBins]; // per tile (S = 8) or per wave
    for (int k = threadIdx.x; k < kWaves * kLtmBins; k += kThreads) {
        (&s_n[0][0])[k] = 0;
        (&s_S[0][0])[k] = 0;
    }
    __syncthreads();
    const int bx0 = blockIdx.x * kRowW, by0 = blockIdx.y * S;
    int cur = -1, slot = threadIdx.x >> 6, run_n = 0, run_S = 0;
#pragma unroll 4
    for (int idx = threadIdx.x; idx < kRowW * S; idx += kThreads) {
        const int px = idx % kRowW, py = idx / kRowW;
        const int x = bx0 + px, y = by0 + py;
        if (x >= a.width || y >= a.height) continue;
        const size_t p = (size_t)y * (size_t)a.width + (size_t)x;
        const float c[3] = { radiance[3 * p], radiance[3 * p + 1], radiance[3 * p + 2] };
        const float l = ltm_luminance(c);
        if (!ltm_mapped(c, l)) continue;
        const int q10 = ltm_q10(ltm_q16(l));
        const int bin = ltm_bin(q10);
        if (kTiles > 1) slot = px / S; // (one pixel per thread: no runs)
        if (bin == cur) {
            ++run_n;
            run_S += q10;
        } else {
            if (cur >= 0) {
                atomicAdd(&s_n[slot][cur], run_n);
                atomicAdd(&s_S[slot][cur], run_S);
            }
            cur = bin;
            run_n = 1;
            run_S = q10;
        }
    }
    if (cur >= 0) {
        atomicAdd(&s_n[slot][cur], run_n);
        atomicAdd(&s_S[slot][cur], run_S);
    }
    __syncthreads();
    if (kTiles > 1) {
        const int tile = threadIdx.x / kLtmBins, z = threadIdx.x % kLtmBins;
        const int cx = blockIdx.x * kTiles + tile;
        if (tile < kTiles && cx < a.gw) {
            LtmCellI v;
            v.n = s_n[tile][z];
            v.S = s_S[tile][z];
            grid[((size_t)blockIdx.y * (size_t)a.gw + (size_t)cx) * kLtmBins + z] = v;
        }
    } else if (threadIdx.x < kLtmBins) {
        const int z = threadIdx.x;
        LtmCellI v;
        v.n = v.S = 0;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) {
            v.n += s_n[w][z];
            v.S += s_S[w][z];
        }
        grid[((size_t)blockIdx.y * (size_t)a.gw + (size_t)blockIdx.x) * kLtmBins + z] = v;
    }
}

__device__ __forceinline__ LtmCellF ltm_load(const LtmCellF* g, size_t i) { return g[i]; }
__device__ __forceinline__ LtmCellF ltm_load(const LtmCellI* g, size_t i)
{
    const LtmCellI v = g[i];
    LtmCellF f;
    f.n = (float)v.n;
    f.S = (float)v.S;
    return f;
}

// AXIS 0: x (reads the integers), 1: y, 2: z.
template <int AXIS, class SRC>
__global__ __launch_bounds__(kThreads) void ltm_blur_kernel(const LtmArgs a, size_t cells, const SRC* __restrict__ src, LtmCellF* __restrict__ dst)
{
    const size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= cells) return;
    const size_t col = i / kLtmBins;
    const int z = (int)(i - col * kLtmBins);
    const int cx = (int)(col % (size_t)a.gw), cy = (int)(col / (size_t)a.gw);
    const size_t stride = AXIS == 0 ? (size_t)kLtmBins : (AXIS == 1 ? (size_t)a.gw * kLtmBins : (size_t)1);
    const int at = AXIS == 0 ? cx : (AXIS == 1 ? cy : z);
    const int last = AXIS == 0 ? a.gw - 1 : (AXIS == 1 ? a.gh - 1 : kLtmBins - 1);
    LtmCellF lo, hi;
    lo.n = lo.S = hi.n = hi.S = 0.0f;
    if (at > 0) lo = ltm_load(src, i - stride);
    if (at < last) hi = ltm_load(src, i + stride);
    const LtmCellF c = ltm_load(src, i);
    LtmCellF v;
    v.n = ltm_blur3(lo.n, c.n, hi.n);
    v.S = ltm_blur3(lo.S, c.S, hi.S);
    dst[i] = v;
}

template <bool COPY>
__global__ __launch_bounds__(kThreads) void ltm_slice_kernel(const LtmArgs a, const float* radiance, const LtmCellF* __restrict__ grid,
                                                             unsigned char* __restrict__ rgb8, float* radiance_out)
{
    const int x = blockIdx.x * kTileW + (threadIdx.x & (kTileW - 1)), y = blockIdx.y * kTileH + threadIdx.x / kTileW;
    if (x >= a.width || y >= a.height) return;
    const size_t p = (size_t)y * (size_t)a.width + (size_t)x;
    const float rad[3] = { radiance[3 * p], radiance[3 * p + 1], radiance[3 * p + 2] };
    float v[3];
    if (COPY) {
        v[0] = rad[0];
        v[1] = rad[1];
        v[2] = rad[2];
    } else {
        ltm_pixel(a, grid, x, y, rad, v);
    }
    store_rgb(p, v, rgb8, radiance_out);
}

template <int S>
void launch_splat(const LtmArgs& a, const float* radiance, LtmCellI* grid, hipStream_t stream)
{
    constexpr int kTiles = S == 8 ? 4 : 1;
    const dim3 blocks((unsigned)((a.gw + kTiles - 1) / kTiles), (unsigned)a.gh);
    hipLaunchKernelGGL((ltm_splat_kernel<S>), blocks, dim3(kThreads), 0, stream, a, radiance, grid);
}

} // namespace

size_t ltm_grid_cells(const LtmArgs& a) { return (size_t)a.gw * (size_t)a.gh * kLtmBins; }

hipError_t launch_local_tonemap(const LtmArgs& a, const float* radiance, void* work, unsigned char* rgb8, float* radiance_out, hipStream_t stream)
{
    if (a.width <= 0 || a.height <= 0) return hipSuccess;
    const dim3 tiles((unsigned)((a.width + kTileW - 1) / kTileW), (unsigned)((a.height + kTileH - 1) / kTileH));
    if (a.identity) {
        if (!rgb8 && (!radiance_out || radiance_out == radiance)) return hipSuccess;
        hipLaunchKernelGGL((ltm_slice_kernel<true>), tiles, dim3(kThreads), 0, stream, a, radiance, (const LtmCellF*)nullptr, rgb8, radiance_out);
        return hipGetLastError();
    }
    const size_t cells = ltm_grid_cells(a);
    LtmCellI* g0i = (LtmCellI*)work;
    LtmCellF* g0 = (LtmCellF*)work;
    LtmCellF* g1 = g0 + cells;
    switch (a.cell) {
    case 8: launch_splat<8>(a, radiance, g0i, stream); break;
    case 16: launch_splat<16>(a, radiance, g0i, stream); break;
    case 32: launch_splat<32>(a, radiance, g0i, stream); break;
    default: launch_splat<64>(a, radiance, g0i, stream); break;
    }
    const dim3 blur((unsigned)((cells + kThreads - 1) / kThreads));
    hipLaunchKernelGGL((ltm_blur_kernel<0, LtmCellI>), blur, dim3(kThreads), 0, stream, a, cells, (const LtmCellI*)g0i, g1);
    hipLaunchKernelGGL((ltm_blur_kernel<1, LtmCellF>), blur, dim3(kThreads), 0, stream, a, cells, (const LtmCellF*)g1, g0);
    hipLaunchKernelGGL((ltm_blur_kernel<2, LtmCellF>), blur, dim3(kThreads), 0, stream, a, cells, (const LtmCellF*)g0, g1);
    hipLaunchKernelGGL((ltm_slice_kernel<false>), tiles, dim3(kThreads), 0, stream, a, radiance, (const LtmCellF*)g1, rgb8, radiance_out);
    return hipGetLastError();
}

} // namespace ff
