// ff_upscale.hip — the kernel behind ff_upscale: G-buffer-guided upsampling of a low-resolution frame.  A translation unit of its
// own beside the other image kernels and the trace kernels, which it does not touch.  The operator is in include/firefly/ff_api.h
// and, as code, in ff_upscale.h (upscale_pixel, which the host twin ff_upscale_host compiles too).
//
// One thread per high pixel, 64 x 4 pixels per workgroup: a wave covers 64 consecutive pixels of one row, so its float3 / int3 guide
// rows and its outputs are runs of 768 (192 for rgb8) contiguous bytes.  The kernel is bandwidth-bound: 48 bytes of guides in and
// 15 out per pixel; the 4 to 16 low taps of a pixel are shared with its neighbours in the wave (a wave's 64 pixels look at 32 + 1
// low columns at factor 2) and come from L1 / L2, so there is no LDS staging.
#include "ff_upscale.h"

namespace ff {
namespace {

__global__ __launch_bounds__(256) void upscale_kernel(const UpscaleArgs a, unsigned char* __restrict__ rgb8, float* __restrict__ radiance_out)
{
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    if (x >= a.width || y >= a.height) return;
    const size_t i = (size_t)y * (size_t)a.width + (size_t)x;
    float v[3];
    upscale_pixel(a, x, y, v);
    if (radiance_out) { radiance_out[3 * i] = v[0]; radiance_out[3 * i + 1] = v[1]; radiance_out[3 * i + 2] = v[2]; }
    if (rgb8) { rgb8[3 * i] = pixel_u8(v[0]); rgb8[3 * i + 1] = pixel_u8(v[1]); rgb8[3 * i + 2] = pixel_u8(v[2]); }
}

} // namespace

hipError_t launch_upscale(const UpscaleArgs& a, unsigned char* rgb8, float* radiance_out, hipStream_t stream)
{
    if (a.width <= 0 || a.height <= 0) return hipSuccess;
    const dim3 grid((unsigned)((a.width + 63) / 64), (unsigned)((a.height + 3) / 4));
    hipLaunchKernelGGL(upscale_kernel, grid, dim3(64, 4), 0, stream, a, rgb8, radiance_out);
    return hipGetLastError();
}

} // namespace ff
