// ff_resize.hip — the kernels behind ff_resize: separable polyphase resampling of a radiance image.  A translation unit of its own
// beside the other image kernels and the trace kernels, which it does not touch.  The operator is in
// include/firefly/ff_api.h and, as code, in ff_resize.h, which the host twin ff_resize_host compiles too.
//
//   resize_h_kernel<RING>   the horizontal pass, W x H -> W' x H.  One workgroup of 256 threads per tile of 64 output columns by
//                           rows_h input rows (4; 2 where the LDS would not hold 4, which only a Lanczos-3 reduction beyond 13 : 1
//                           reaches), a wave on a row, a lane on an output column.  The tile's outputs name one contiguous span of
//                           input columns (first is monotone and so is the clamp): each wave copies its row's span into LDS with
//                           coalesced dword loads, a non-finite sample becoming +0 on the way, and all four stage the tile's
//                           weights, tap-major, so that a tap's 64 weights are 64 consecutive words.  After one barrier a lane walks
//                           its T taps out of LDS: the overlapping, unaligned reads of neighbouring outputs never reach L2, and
//                           HBM sees the input once (plus the few columns two tiles share).
//   resize_v_kernel<RING>   the vertical pass, W' x H -> W' x H'.  One workgroup of 256 threads per tile of 64 columns by 16 output
//                           rows, a lane on a column, a wave on four consecutive output rows, one after the other.  A tap reads
//                           one row of the intermediate image: 64 lanes, 768 consecutive bytes.  Nothing is staged: the rows that
//                           consecutive outputs share come back from L1 / L2 (a tile's rows at the limits would be 270 KB, no LDS
//                           holds them), and the weights and first of a row are the same for the whole wave and come through
//                           scalar loads.
//                           RING = FF_RESIZE_ANTI_RING: two instantiations each.
#include "ff_resize.h"

namespace ff {
namespace {

constexpr int kThreads = 256, kWaves = kThreads / 64;
static_assert(kResizeTileX == 64, "a lane per output column of the tile");
static_assert(kResizeRowsV == 4 * kWaves, "a wave on four output rows");

template <bool RING>
__global__ __launch_bounds__(kThreads) void resize_h_kernel(const ResizeArgs a, const float* __restrict__ radiance, float* __restrict__ mid)
{
    extern __shared__ float s_mem[]; // rows_h spans of 3 * a.x.span floats, then taps * 64 weights
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n = a.x.in_size, N = a.x.out_size, T = a.x.taps, H = a.y.in_size;
    const int X0 = blockIdx.x * kResizeTileX;
    const int X1 = X0 + kResizeTileX < N ? X0 + kResizeTileX : N;
    // the span of input columns the tile's outputs name: [s0, s0 + len)
    const int s0 = resize_index(a.x.first[X0], 0, n);
    const int len = resize_index(a.x.first[X1 - 1], T - 1, n) - s0 + 1;
    if (len > a.x.span) return; // (the host sized the LDS from the same table: never taken)
    float* s_w = s_mem + (size_t)a.rows_h * 3 * a.x.span;
    for (int i = threadIdx.x; i < T * kResizeTileX; i += kThreads) {
        const int x = X0 + (i & (kResizeTileX - 1));
        s_w[i] = x < N ? a.x.weights[(size_t)(i / kResizeTileX) * N + x] : 0.f;
    }
    const int y0 = blockIdx.y * a.rows_h;
    for (int r = wave; r < a.rows_h && y0 + r < H; r += kWaves) {
        const float* src = radiance + ((size_t)(y0 + r) * n + s0) * 3;
        float* row = s_mem + (size_t)r * 3 * a.x.span;
        for (int i = lane; i < 3 * len; i += 64) row[i] = resize_value(src[i]);
    }
    __syncthreads();

    const int X = X0 + lane;
    if (X >= N) return;
    const int first = a.x.first[X];
    for (int r = wave; r < a.rows_h && y0 + r < H; r += kWaves) {
        const float* row = s_mem + (size_t)r * 3 * a.x.span;
        ResizeSum s[3] = { resize_begin(), resize_begin(), resize_begin() };
        for (int j = 0; j < T; ++j) {
            const float w = s_w[j * kResizeTileX + lane];
            const float* v = row + 3 * (resize_index(first, j, n) - s0);
            resize_tap<RING>(s[0], w, v[0]);
            resize_tap<RING>(s[1], w, v[1]);
            resize_tap<RING>(s[2], w, v[2]);
        }
        float* o = mid + ((size_t)(y0 + r) * N + X) * 3;
        o[0] = resize_finish<RING>(s[0]);
        o[1] = resize_finish<RING>(s[1]);
        o[2] = resize_finish<RING>(s[2]);
    }
}

template <bool RING>
__global__ __launch_bounds__(kThreads) void resize_v_kernel(const ResizeArgs a, const float* __restrict__ mid, unsigned char* __restrict__ rgb8,
                                                            float* __restrict__ radiance_out)
{
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6); // (the same in every lane: the row's table comes through scalar loads)
    const int N = a.x.out_size, n = a.y.in_size, NY = a.y.out_size, T = a.y.taps;
    const int X = blockIdx.x * kResizeTileX + lane;
    if (X >= N) return;
    const int Y0 = blockIdx.y * kResizeRowsV + wave * (kResizeRowsV / kWaves);
    for (int Y = Y0; Y < Y0 + kResizeRowsV / kWaves && Y < NY; ++Y) {
        const int first = a.y.first[Y];
        const float* w = a.y.weights + (size_t)Y * T;
        ResizeSum s[3] = { resize_begin(), resize_begin(), resize_begin() };
#pragma unroll 4
        for (int j = 0; j < T; ++j) { // (four rows' loads in flight)
            const float* v = mid + ((size_t)resize_index(first, j, n) * N + X) * 3;
            const float wj = w[j];
            resize_tap<RING>(s[0], wj, resize_value(v[0]));
            resize_tap<RING>(s[1], wj, resize_value(v[1]));
            resize_tap<RING>(s[2], wj, resize_value(v[2]));
        }
        const float out[3] = { resize_finish<RING>(s[0]), resize_finish<RING>(s[1]), resize_finish<RING>(s[2]) };
        store_rgb((size_t)Y * N + X, out, rgb8, radiance_out);
    }
}

template <bool RING>
void launch(const ResizeArgs& a, const float* radiance, float* mid, unsigned char* rgb8, float* radiance_out, hipStream_t stream)
{
    const unsigned tiles_x = (unsigned)((a.x.out_size + kResizeTileX - 1) / kResizeTileX);
    const dim3 grid_h(tiles_x, (unsigned)((a.y.in_size + a.rows_h - 1) / a.rows_h));
    const dim3 grid_v(tiles_x, (unsigned)((a.y.out_size + kResizeRowsV - 1) / kResizeRowsV));
    hipLaunchKernelGGL((resize_h_kernel<RING>), grid_h, dim3(kThreads), resize_lds_bytes(a.rows_h, a.x.span, a.x.taps), stream, a, radiance, mid);
    hipLaunchKernelGGL((resize_v_kernel<RING>), grid_v, dim3(kThreads), 0, stream, a, mid, rgb8, radiance_out);
}

} // namespace

hipError_t launch_resize(const ResizeArgs& a, const float* radiance, float* mid, unsigned char* rgb8, float* radiance_out, hipStream_t stream)
{
    if (a.x.in_size <= 0 || a.y.in_size <= 0 || a.x.out_size <= 0 || a.y.out_size <= 0) return hipSuccess;
    if ((a.rows_h != kResizeRowsH && a.rows_h != kResizeRowsHSmall) || a.x.span < 1 || a.x.taps < 1 || a.y.taps < 1 ||
        resize_lds_bytes(a.rows_h, a.x.span, a.x.taps) > kResizeLdsBytes)
        return hipErrorInvalidValue;
    if (a.anti_ring)
        launch<true>(a, radiance, mid, rgb8, radiance_out, stream);
    else
        launch<false>(a, radiance, mid, rgb8, radiance_out, stream);
    return hipGetLastError();
}

} // namespace ff
