// ff_sharpen.hip — the kernel behind ff_sharpen: contrast-adaptive sharpening of a radiance image.  A translation unit of its own
// beside the other image kernels and the trace kernels, which it does not touch.  The operator is in
// include/firefly/ff_api.h and, as code, in ff_sharpen.h, which the host twin ff_sharpen_host compiles too.
//
//   sharpen_kernel<NOISE>   one workgroup of 256 threads per tile of 32 x 8 pixels, a wave on two rows of 32 (ff_despeckle's shape).
//                           Step 1 (the three divisions and the luminance) is fused into the load: a thread compresses its own
//                           pixel into one 16-byte cell {t_r, t_g, t_b, L} in LDS and keeps the raw radiance in registers for the
//                           copy-through; the first 80 threads then fill the cross apron - the row above, the row below and the
//                           column on each side, no corners.  The cells stand in rows of 34 (the four corners are there and are
//                           never touched): 340 cells, 5440 bytes.  L carries the marks of an unusable pixel and of a cell outside
//                           the image, so step 2's rule reads nothing else.  After one barrier a thread reads its four taps at
//                           constant offsets from its own cell - 16-byte reads of 32 consecutive cells per half wave, which no
//                           lane group of such a read shares a bank in - and finishes in registers.
//                           NOISE = FF_SHARPEN_NOISE_AWARE: two instantiations.
#include "ff_sharpen.h"

namespace ff {
namespace {

constexpr int kTileW = 32, kTileH = 8, kThreads = kTileW * kTileH;
constexpr int kW = kTileW + 2, kH = kTileH + 2;       // the tile with its apron
constexpr int kApron = 2 * kTileW + 2 * kTileH;       // the cross apron's cells

// One cell out of LDS as one 16-byte read.
__device__ __forceinline__ SharpenCell read_cell(const SharpenCell* c)
{
    const float4 q = *reinterpret_cast<const float4*>(c);
    SharpenCell s;
    s.t[0] = q.x;
    s.t[1] = q.y;
    s.t[2] = q.z;
    s.l = q.w;
    return s;
}

template <bool NOISE>
__global__ __launch_bounds__(kThreads) void sharpen_kernel(const SharpenArgs a, const float* __restrict__ radiance, unsigned char* __restrict__ rgb8,
                                                           float* __restrict__ radiance_out)
{
    __shared__ SharpenCell s_cell[kW * kH];
    const int tx = threadIdx.x & (kTileW - 1), ty = threadIdx.x / kTileW;
    const int x0 = blockIdx.x * kTileW - 1, y0 = blockIdx.y * kTileH - 1; // the image position of cell (0, 0)
    SharpenCell outside;
    outside.t[0] = outside.t[1] = outside.t[2] = 0.f;
    outside.l = kSharpenOutside;

    // the thread's own pixel: cell (tx + 1, ty + 1)
    const int x = x0 + 1 + tx, y = y0 + 1 + ty;
    const bool inside = x < a.width && y < a.height;
    const size_t p = (size_t)y * (size_t)a.width + (size_t)x;
    float rad[3] = { 0.f, 0.f, 0.f };
    SharpenCell E = outside;
    if (inside) {
        rad[0] = radiance[3 * p];
        rad[1] = radiance[3 * p + 1];
        rad[2] = radiance[3 * p + 2];
        E = sharpen_compress(rad);
    }
    SharpenCell* own = s_cell + (ty + 1) * kW + (tx + 1);
    *own = E;
    // the apron: the row above, the row below, the column to the left, the column to the right
    if (threadIdx.x < kApron) {
        const int i = threadIdx.x;
        int cx, cy;
        if (i < 2 * kTileW) {
            cx = 1 + (i & (kTileW - 1));
            cy = i < kTileW ? 0 : kH - 1;
        } else {
            const int j = i - 2 * kTileW;
            cx = j < kTileH ? 0 : kW - 1;
            cy = 1 + (j & (kTileH - 1));
        }
        const int qx = x0 + cx, qy = y0 + cy;
        SharpenCell Y = outside;
        if (qx >= 0 && qy >= 0 && qx < a.width && qy < a.height) {
            const size_t q = (size_t)qy * (size_t)a.width + (size_t)qx;
            const float c3[3] = { radiance[3 * q], radiance[3 * q + 1], radiance[3 * q + 2] };
            Y = sharpen_compress(c3);
        }
        s_cell[cy * kW + cx] = Y;
    }
    __syncthreads();

    if (!inside) return;
    const SharpenCell B = read_cell(own - kW), D = read_cell(own - 1), F = read_cell(own + 1), H = read_cell(own + kW);
    float v[3];
    sharpen_pixel<NOISE>(a.strength, E, B, D, F, H, rad, v);
    store_rgb(p, v, rgb8, radiance_out);
}

template <bool NOISE>
void launch(const SharpenArgs& a, const float* radiance, unsigned char* rgb8, float* radiance_out, hipStream_t stream)
{
    const dim3 grid((unsigned)((a.width + kTileW - 1) / kTileW), (unsigned)((a.height + kTileH - 1) / kTileH));
    hipLaunchKernelGGL((sharpen_kernel<NOISE>), grid, dim3(kThreads), 0, stream, a, radiance, rgb8, radiance_out);
}

} // namespace

hipError_t launch_sharpen(const SharpenArgs& a, const float* radiance, unsigned char* rgb8, float* radiance_out, hipStream_t stream)
{
    if (a.width <= 0 || a.height <= 0) return hipSuccess;
    if (a.noise_aware)
        launch<true>(a, radiance, rgb8, radiance_out, stream);
    else
        launch<false>(a, radiance, rgb8, radiance_out, stream);
    return hipGetLastError();
}

} // namespace ff
