// ff_tile_filter.h — the skeleton ff_motion_blur and ff_depth_of_field share: (1) pack a per-pixel record, (2) every k x k tile's
// maximum T, (3) the 3 x 3 neighbour maximum N, (4) a gather along or inside that radius into radiance_out and rgb8.  A filter
// describes itself with a policy struct F in its own header (MotionBlurFilter, DofFilter):
//
//   Args, Packed, Tile, Key      the kernel arguments (with a TileGrid `grid`), a pixel's record, a tile's, and the reduction key
//   kGuideFloats, kGatherRoom    floats per pixel of the guide plane beside depth; bytes of room per pixel the gather wants
//   kUniqueKey                   true: no two pixels of a tile share a key, and whoever holds the winner writes T = tile_of(its
//                                record).  false: the key is T itself, ties are harmless, and one lane alone writes it
//   lowest_key()                 below (or equal to) every pixel's key
//   pack(a, guide, depth)        step 1;  key(packed, index_in_tile);  tile_of(packed)
//   neighbour_max(a, T, tx, ty)  step 3;  gather(a, x, y, plane, radiance, n, room, stride, out)  step 4
//   launch_gather(...)           its own gather kernel (the filter's .hip), launched through launch_gather_kernel
//
// and its .hip unit instantiates launch_pack_tile_max<F> and launch_neighbour_max<F>.  The host half - the work buffer and the
// staging, the three launches, and the host twin's three loops over the same per-pixel functions - is tile_filter_device<F> and
// tile_filter_host<F>.  Every output is a function of its own inputs alone: nothing depends on the order of floating-point adds
// or of the workgroups.
#pragma once

#include <array>
#include <string>
#include <type_traits>
#include <vector>

#include "ff_pixel.h"
#include "ff_state.h"

namespace ff {

// Images are row-major, top row first; tile (tx, ty) covers the pixels from (tx k, ty k) on, fewer at the right and bottom edges.
struct TileGrid {
    int width, height;
    int k;                // the tile edge (max_radius)
    int tiles_x, tiles_y; // ceil(width / k), ceil(height / k)
};

inline TileGrid make_tile_grid(int width, int height, int k) { return { width, height, k, (width + k - 1) / k, (height + k - 1) / k }; }

FF_PIXEL_HD size_t tile_count(const TileGrid& g) { return (size_t)g.tiles_x * (size_t)g.tiles_y; }

// Whether tile (tx, ty) has a pixel of row-major index i (in the tile); *p: that pixel's index in the image.
FF_PIXEL_HD bool tile_pixel(const TileGrid& g, int tx, int ty, int i, size_t* p)
{
    const int x0 = tx * g.k, y0 = ty * g.k;
    const int tw = g.k < g.width - x0 ? g.k : g.width - x0, th = g.k < g.height - y0 ? g.k : g.height - y0;
    const int ly = i / tw, lx = i - ly * tw;
    *p = (size_t)(y0 + ly) * (size_t)g.width + (size_t)(x0 + lx);
    return i < tw * th;
}

// The tile of pixel (x, y), as an index into T and N.
FF_PIXEL_HD size_t tile_of_pixel(const TileGrid& g, int x, int y) { return (size_t)(y / g.k) * (size_t)g.tiles_x + (size_t)(x / g.k); }

// (a) step 1 into plane (W*H Packed) and step 2 into tile_max (tiles_x * tiles_y Tile): one workgroup per tile, or for k <= 8 a
// group of lanes per tile.  (b) step 3: neighbour_max from tile_max.  Defined below for the filter's .hip unit to instantiate.
template <class F>
hipError_t launch_pack_tile_max(const typename F::Args& a, const float* guide, const float* depth, typename F::Packed* plane, typename F::Tile* tile_max,
                                hipStream_t stream);
template <class F>
hipError_t launch_neighbour_max(const typename F::Args& a, const typename F::Tile* tile_max, typename F::Tile* neighbour_max, hipStream_t stream);

#if defined(__HIPCC__)

namespace { // (internal linkage, as every kernel of the library has: the unit that instantiates a kernel is the one that launches it)

constexpr int kTileThreads = 256;

// The largest key among GROUP consecutive lanes (a power of two, at most a wave), in every one of them.
template <int GROUP, class Key>
__device__ __forceinline__ Key lane_group_max(Key win)
{
#pragma unroll
    for (int off = GROUP / 2; off >= 1; off >>= 1) {
        const Key other = __shfl_xor(win, off, 64);
        win = other > win ? other : win;
    }
    return win;
}

// (a) for k > 8, one workgroup of 256 threads per tile: every thread packs its pixels into the plane and keeps the largest key
// among them; the keys meet in a wave-level max, then across the four waves through LDS.
template <class F>
__global__ __launch_bounds__(kTileThreads) void pack_tile_max_kernel(const typename F::Args a, const float* __restrict__ guide, const float* __restrict__ depth,
                                                                     typename F::Packed* __restrict__ plane, typename F::Tile* __restrict__ tile_max)
{
    using Key = typename F::Key;
    __shared__ Key s_key[kTileThreads / 64];
    Key best = F::lowest_key();
    typename F::Packed best_p = {};
    size_t p;
    for (int i = threadIdx.x; tile_pixel(a.grid, blockIdx.x, blockIdx.y, i, &p); i += kTileThreads) {
        const typename F::Packed v = F::pack(a, guide + F::kGuideFloats * p, depth[p]);
        plane[p] = v;
        const Key key = F::key(v, (unsigned)i);
        if (key > best) {
            best = key;
            best_p = v;
        }
    }
    Key win = lane_group_max<64>(best);
    if ((threadIdx.x & 63) == 0) s_key[threadIdx.x >> 6] = win;
    __syncthreads();
    const size_t tile = (size_t)blockIdx.y * (size_t)a.grid.tiles_x + (size_t)blockIdx.x;
    if constexpr (F::kUniqueKey) {
        for (int w = 0; w < kTileThreads / 64; ++w) win = s_key[w] > win ? s_key[w] : win;
        if (best == win) tile_max[tile] = F::tile_of(best_p);
    } else if (threadIdx.x == 0) {
        for (int w = 1; w < kTileThreads / 64; ++w) win = s_key[w] > win ? s_key[w] : win;
        tile_max[tile] = win;
    }
}

// (a) for tiles of at most 64 pixels (k <= 8): a group of P = GROUP consecutive lanes per tile, P the power of two that holds k * k,
// 256 / P tiles per workgroup in row-major order of the tiles.  Lane i of a group packs the tile's pixel i; the keys meet in log2 P
// shuffle steps that stay inside the group.  No LDS, no idle waves: at k = 1 a lane is a tile and consecutive lanes are
// consecutive pixels.
template <class F, int GROUP>
__global__ __launch_bounds__(kTileThreads) void pack_small_tiles_kernel(const typename F::Args a, const float* __restrict__ guide,
                                                                        const float* __restrict__ depth, typename F::Packed* __restrict__ plane,
                                                                        typename F::Tile* __restrict__ tile_max)
{
    const size_t tiles = tile_count(a.grid);
    const size_t tile = (size_t)blockIdx.x * (kTileThreads / GROUP) + threadIdx.x / GROUP;
    const int i = threadIdx.x % GROUP;
    typename F::Key best = F::lowest_key(); // (a lane without a pixel)
    typename F::Packed v = {};
    size_t p;
    if (tile < tiles && tile_pixel(a.grid, (int)(tile % (size_t)a.grid.tiles_x), (int)(tile / (size_t)a.grid.tiles_x), i, &p)) {
        v = F::pack(a, guide + F::kGuideFloats * p, depth[p]);
        plane[p] = v;
        best = F::key(v, (unsigned)i);
    }
    const typename F::Key win = lane_group_max<GROUP>(best);
    if constexpr (F::kUniqueKey) {
        if (best != F::lowest_key() && best == win) tile_max[tile] = F::tile_of(v);
    } else if (i == 0 && tile < tiles) {
        tile_max[tile] = win;
    }
}

template <class F, int GROUP>
void launch_small_tiles(const typename F::Args& a, const float* guide, const float* depth, typename F::Packed* plane, typename F::Tile* tile_max,
                        hipStream_t stream)
{
    const size_t per_block = kTileThreads / GROUP;
    hipLaunchKernelGGL((pack_small_tiles_kernel<F, GROUP>), dim3((unsigned)((tile_count(a.grid) + per_block - 1) / per_block)), dim3(kTileThreads), 0, stream,
                       a, guide, depth, plane, tile_max);
}

} // namespace

template <class F>
hipError_t launch_pack_tile_max(const typename F::Args& a, const float* guide, const float* depth, typename F::Packed* plane, typename F::Tile* tile_max,
                                hipStream_t stream)
{
    static_assert(F::kUniqueKey || std::is_same<typename F::Key, typename F::Tile>::value, "a key that can tie is the tile's record itself");
    if (a.grid.width <= 0 || a.grid.height <= 0) return hipSuccess;
    // a tile of at most 64 pixels is the work of a part of a wave: several tiles per workgroup
    const int pixels = a.grid.k * a.grid.k;
    if (pixels <= 1) launch_small_tiles<F, 1>(a, guide, depth, plane, tile_max, stream);
    else if (pixels <= 4) launch_small_tiles<F, 4>(a, guide, depth, plane, tile_max, stream);
    else if (pixels <= 16) launch_small_tiles<F, 16>(a, guide, depth, plane, tile_max, stream);
    else if (pixels <= 32) launch_small_tiles<F, 32>(a, guide, depth, plane, tile_max, stream);
    else if (pixels <= 64) launch_small_tiles<F, 64>(a, guide, depth, plane, tile_max, stream);
    else hipLaunchKernelGGL(pack_tile_max_kernel<F>, dim3((unsigned)a.grid.tiles_x, (unsigned)a.grid.tiles_y), dim3(kTileThreads), 0, stream, a, guide, depth, plane, tile_max);
    return hipGetLastError();
}

namespace {

// (b) one thread per tile.
template <class F>
__global__ __launch_bounds__(256) void neighbour_max_kernel(const typename F::Args a, const typename F::Tile* __restrict__ tile_max,
                                                            typename F::Tile* __restrict__ neighbour_max)
{
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= tile_count(a.grid)) return;
    neighbour_max[t] = F::neighbour_max(a, tile_max, (int)(t % (size_t)a.grid.tiles_x), (int)(t / (size_t)a.grid.tiles_x));
}

} // namespace

template <class F>
hipError_t launch_neighbour_max(const typename F::Args& a, const typename F::Tile* tile_max, typename F::Tile* neighbour_max, hipStream_t stream)
{
    const size_t tiles = tile_count(a.grid);
    if (tiles == 0) return hipSuccess;
    hipLaunchKernelGGL(neighbour_max_kernel<F>, dim3((unsigned)((tiles + 255) / 256)), dim3(256), 0, stream, a, tile_max, neighbour_max);
    return hipGetLastError();
}

// (c) a filter's gather kernel: one thread per pixel, 64 x 4 pixels per workgroup, a wave on 64 consecutive pixels of a row
// (x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y).
template <class Kernel, class Args, class... Buffers>
hipError_t launch_gather_kernel(Kernel kernel, const Args& a, hipStream_t stream, Buffers... buffers)
{
    if (a.grid.width <= 0 || a.grid.height <= 0) return hipSuccess;
    const dim3 grid((unsigned)((a.grid.width + 63) / 64), (unsigned)((a.grid.height + 3) / 4));
    hipLaunchKernelGGL(kernel, grid, dim3(64, 4), 0, stream, a, buffers...);
    return hipGetLastError();
}

#endif // __HIPCC__

// The device entry point behind the checks: the filter's use of the state's image work buffer (the packed plane, T and N, then,
// from a multiple of 16 bytes on, the staging of host buffers), the three launches, the wait.  rgb8 and radiance_out may be null.
template <class F>
int tile_filter_device(FfState* s, const typename F::Args& a, const float* radiance_in, const float* guide, const float* depth, int inputs_on_device,
                       void* rgb8, int rgb8_on_device, float* radiance_out, int radiance_out_on_device, const char* who)
{
    FF_HIP(hipSetDevice(s->device));
    hipStream_t stream = s->stream;
    const size_t px = (size_t)a.grid.width * (size_t)a.grid.height, tiles = tile_count(a.grid);
    const size_t own_bytes = (px * sizeof(typename F::Packed) + 2 * tiles * sizeof(typename F::Tile) + 15) & ~(size_t)15;
    Staging stage(&s->d_img_work, &s->img_work_bytes, own_bytes);
    if (!inputs_on_device) {
        stage.in(&radiance_in, radiance_in, px * 12);
        stage.in(&guide, guide, px * 4 * F::kGuideFloats);
        stage.in(&depth, depth, px * 4);
    }
    StagedOutputs out(stage, px, rgb8, rgb8_on_device, radiance_out, radiance_out_on_device);
    const int st = stage.commit(stream, (std::string(who) + ": staging the inputs failed").c_str());
    if (st != FF_OK) return st;
    typename F::Packed* plane = (typename F::Packed*)s->d_img_work;
    typename F::Tile* tile_max = (typename F::Tile*)(plane + px);
    typename F::Tile* neighbour_max = tile_max + tiles;
    FF_HIP(launch_pack_tile_max<F>(a, guide, depth, plane, tile_max, stream));
    FF_HIP(launch_neighbour_max<F>(a, tile_max, neighbour_max, stream));
    if (out.rgb8 || out.radiance) FF_HIP(F::launch_gather(a, plane, neighbour_max, radiance_in, out.rgb8, out.radiance, stream));
    FF_HIP(hipStreamSynchronize(stream));
    return stage.finish();
}

// The host twin: the same per-pixel functions in loops.
template <class F>
void tile_filter_host(const typename F::Args& a, const float* radiance_in, const float* guide, const float* depth, unsigned char* rgb8, float* radiance_out)
{
    const TileGrid& g = a.grid;
    std::vector<typename F::Packed> plane((size_t)g.width * (size_t)g.height);
    std::vector<typename F::Tile> tile_max(tile_count(g)), neighbour_max(tile_count(g));
    // steps 1 and 2: a tile's pixels in row-major order, a later one replaces the best only when its key is larger
    for (int ty = 0; ty < g.tiles_y; ++ty)
        for (int tx = 0; tx < g.tiles_x; ++tx) {
            typename F::Key best = F::lowest_key();
            typename F::Packed best_p = {};
            size_t q;
            for (int i = 0; tile_pixel(g, tx, ty, i, &q); ++i) {
                const typename F::Packed v = F::pack(a, guide + F::kGuideFloats * q, depth[q]);
                plane[q] = v;
                const typename F::Key key = F::key(v, (unsigned)i);
                if (key > best) {
                    best = key;
                    best_p = v;
                }
            }
            tile_max[(size_t)ty * (size_t)g.tiles_x + (size_t)tx] = F::tile_of(best_p);
        }
    for (int ty = 0; ty < g.tiles_y; ++ty)
        for (int tx = 0; tx < g.tiles_x; ++tx) neighbour_max[(size_t)ty * (size_t)g.tiles_x + (size_t)tx] = F::neighbour_max(a, tile_max.data(), tx, ty);
    std::array<signed char, F::kGatherRoom> room;
    for (int y = 0; y < g.height; ++y)
        for (int x = 0; x < g.width; ++x) {
            float v[3];
            F::gather(a, x, y, plane.data(), radiance_in, neighbour_max[tile_of_pixel(g, x, y)], room.data(), 1, v);
            store_rgb((size_t)y * (size_t)g.width + (size_t)x, v, rgb8, radiance_out);
        }
}

} // namespace ff
