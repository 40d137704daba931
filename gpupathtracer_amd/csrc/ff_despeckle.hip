// ff_despeckle.hip — the kernel behind ff_despeckle: a G-buffer-guided firefly clamp.  A translation unit of its own beside the
// other image kernels and the trace kernels, which it does not touch.  The operator is in
// include/firefly/ff_api.h and, as code, in ff_despeckle.h, which the host twin ff_despeckle_host compiles too.
//
//   despeckle_kernel<R, RANK>   one workgroup of 256 threads per tile of 32 x 8 pixels, a wave on two rows of 32.  Step 1 (the three
//                               divisions and the luminance) is fused into the load of the tile and its apron of R pixels into
//                               LDS, one {l, g} of 8 bytes per pixel, g = -1 where the pixel does not count or lies outside the
//                               image: a thread measures its own pixel first and keeps the radiance, then the threads share the
//                               apron.  After one barrier a thread walks its (2R+1)^2 window in LDS - rows of 32 consecutive
//                               8-byte cells per half wave: no bank conflict - and keeps the RANK largest luminances in a sorted
//                               list that is unrolled into registers.  A clamped lane reads its albedo again for step 3's measure of the output.  The clamped pixels are counted per wave (ballot, popcount),
//                               summed over the workgroup's four waves in LDS, and leave as one atomicAdd of an integer per
//                               workgroup into one of kDespeckleSlots counters, each on a cache line of its own, that the host
//                               adds up: integer sums, whatever the order.  (One counter for all waves made the call's time that
//                               of 32 000 atomics on one address at 1080p: DESIGN.md section 8 row 18.)
//                               R = 1 .. 3 and RANK = 1 .. 4: twelve instantiations.
#include "ff_despeckle.h"

namespace ff {
namespace {

constexpr int kTileW = 32, kTileH = 8, kThreads = kTileW * kTileH;

template <int R, int RANK>
__global__ __launch_bounds__(kThreads) void despeckle_kernel(const DespeckleArgs a, const float* __restrict__ radiance, const float* __restrict__ albedo,
                                                             const int32_t* __restrict__ ids, unsigned char* __restrict__ rgb8,
                                                             float* __restrict__ radiance_out, uint32_t* __restrict__ clamped)
{
    constexpr int kW = kTileW + 2 * R, kH = kTileH + 2 * R; // the tile with its apron
    constexpr int kBand = 2 * R * kW;                        // the apron's cells above and below the tile
    constexpr int kApron = kW * kH - kThreads;
    __shared__ DespeckleCell s_cell[kW * kH];
    __shared__ uint32_t s_count;
    if (threadIdx.x == 0) s_count = 0;
    const int tx = threadIdx.x & (kTileW - 1), ty = threadIdx.x / kTileW;
    const int x0 = blockIdx.x * kTileW - R, y0 = blockIdx.y * kTileH - R; // the image position of cell (0, 0)
    const DespeckleCell outside = { 0.f, -1 };

    // the thread's own pixel: cell (tx + R, ty + R)
    const int x = x0 + R + tx, y = y0 + R + ty;
    const bool inside = x < a.width && y < a.height;
    const size_t p = (size_t)y * (size_t)a.width + (size_t)x;
    float rad[3] = { 0.f, 0.f, 0.f };
    DespeckleCell X = outside;
    if (inside) {
        rad[0] = radiance[3 * p];
        rad[1] = radiance[3 * p + 1];
        rad[2] = radiance[3 * p + 2];
        X = despeckle_measure(rad, a.demodulate ? albedo + 3 * p : nullptr, ids + 3 * p);
    }
    s_cell[(ty + R) * kW + (tx + R)] = X;
    // the apron: R full rows above, R below, then R cells left and right of each of the tile's rows
    for (int i = threadIdx.x; i < kApron; i += kThreads) {
        int cx, cy;
        if (i < kBand) {
            const int row = i / kW;
            cx = i - row * kW;
            cy = row < R ? row : row + kTileH;
        } else {
            const int j = i - kBand, row = j / (2 * R), c = j - row * (2 * R);
            cx = c < R ? c : c + kTileW;
            cy = R + row;
        }
        const int qx = x0 + cx, qy = y0 + cy;
        DespeckleCell Y = outside;
        if (qx >= 0 && qy >= 0 && qx < a.width && qy < a.height) {
            const size_t q = (size_t)qy * (size_t)a.width + (size_t)qx;
            const float c3[3] = { radiance[3 * q], radiance[3 * q + 1], radiance[3 * q + 2] };
            Y = despeckle_measure(c3, a.demodulate ? albedo + 3 * q : nullptr, ids + 3 * q);
        }
        s_cell[cy * kW + cx] = Y;
    }
    __syncthreads();

    DespeckleTop<RANK> top;
    despeckle_begin(top);
    const DespeckleCell* window = s_cell + ty * kW + tx; // the window's top-left cell
#pragma unroll
    for (int dy = 0; dy <= 2 * R; ++dy)
#pragma unroll
        for (int dx = 0; dx <= 2 * R; ++dx)
            if (dx != R || dy != R) despeckle_take(top, X, window[dy * kW + dx]);
    float v[3];
    const bool hit = despeckle_clamp(a, X, top, rad, a.demodulate ? albedo + 3 * p : nullptr, v) && inside;
    if (inside) store_rgb(p, v, rgb8, radiance_out);
    const unsigned long long votes = __ballot(hit);
    if ((threadIdx.x & 63) == 0 && votes != 0) atomicAdd(&s_count, (uint32_t)__popcll(votes));
    __syncthreads();
    if (threadIdx.x == 0 && s_count != 0) {
        const unsigned slot = (blockIdx.y * gridDim.x + blockIdx.x) & (kDespeckleSlots - 1);
        atomicAdd(clamped + slot * kDespeckleSlotStride, s_count);
    }
}

template <int R, int RANK>
void launch(const DespeckleArgs& a, const float* radiance, const float* albedo, const int32_t* ids, unsigned char* rgb8, float* radiance_out, uint32_t* clamped,
            hipStream_t stream)
{
    const dim3 grid((unsigned)((a.width + kTileW - 1) / kTileW), (unsigned)((a.height + kTileH - 1) / kTileH));
    hipLaunchKernelGGL((despeckle_kernel<R, RANK>), grid, dim3(kThreads), 0, stream, a, radiance, albedo, ids, rgb8, radiance_out, clamped);
}

template <int R>
bool launch_rank(const DespeckleArgs& a, const float* radiance, const float* albedo, const int32_t* ids, unsigned char* rgb8, float* radiance_out,
                 uint32_t* clamped, hipStream_t stream)
{
    switch (a.rank) {
    case 1: launch<R, 1>(a, radiance, albedo, ids, rgb8, radiance_out, clamped, stream); return true;
    case 2: launch<R, 2>(a, radiance, albedo, ids, rgb8, radiance_out, clamped, stream); return true;
    case 3: launch<R, 3>(a, radiance, albedo, ids, rgb8, radiance_out, clamped, stream); return true;
    case 4: launch<R, 4>(a, radiance, albedo, ids, rgb8, radiance_out, clamped, stream); return true;
    }
    return false;
}

} // namespace

hipError_t launch_despeckle(const DespeckleArgs& a, const float* radiance, const float* albedo, const int32_t* ids, unsigned char* rgb8, float* radiance_out,
                            uint32_t* clamped, hipStream_t stream)
{
    if (a.width <= 0 || a.height <= 0) return hipSuccess;
    bool known = false;
    switch (a.radius) {
    case 1: known = launch_rank<1>(a, radiance, albedo, ids, rgb8, radiance_out, clamped, stream); break;
    case 2: known = launch_rank<2>(a, radiance, albedo, ids, rgb8, radiance_out, clamped, stream); break;
    case 3: known = launch_rank<3>(a, radiance, albedo, ids, rgb8, radiance_out, clamped, stream); break;
    }
    return known ? hipGetLastError() : hipErrorInvalidValue; // (a missing instantiation is an error, never a fallback)
}

} // namespace ff
