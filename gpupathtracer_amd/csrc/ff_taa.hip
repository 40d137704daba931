// ff_taa.hip — the temporal anti-aliasing resolve behind ff_taa (Karis 2014, Salvi 2016).  A translation unit of its own beside
// ff_denoise.hip, ff_temporal.hip and the trace kernels, which it does not touch.  The formulas are
// in include/firefly/ff_api.h.
//
// One launch per call: 16x16-pixel workgroups.  The workgroup's 18x18 tile of radiance (its one-pixel apron clamped at the image
// borders) is staged in LDS for the 3x3 clamp statistics; the history taps are float4 loads {rgb, len} from the buffer the
// previous call wrote.  No atomics, no cross-workgroup waits: every output is a function of the inputs and the history alone.
// The motion, the resampling and the clamp box are ff_taa_common.h's, shared with ff_taa_upscale.hip.
#include "ff_taa_common.h"

namespace ff {
namespace {

constexpr int kTile = 16;
constexpr int kApron = kTile + 2;

__global__ __launch_bounds__(256) void taa_kernel(const TaaArgs a, const float* __restrict__ radiance, const float* __restrict__ position,
                                                  const int* __restrict__ ids, unsigned char* __restrict__ rgb8, float* __restrict__ radiance_out)
{
    __shared__ float s_c[3][kApron][kApron];
    const int W = a.width, H = a.height;
    const int tx = threadIdx.x & (kTile - 1), ty = threadIdx.x / kTile;
    const int x = blockIdx.x * kTile + tx, y = blockIdx.y * kTile + ty;
    for (int k = threadIdx.x; k < kApron * kApron; k += kTile * kTile) {
        const int gx = min(max((int)blockIdx.x * kTile - 1 + k % kApron, 0), W - 1);
        const int gy = min(max((int)blockIdx.y * kTile - 1 + k / kApron, 0), H - 1);
        const size_t j = (size_t)gy * (size_t)W + (size_t)gx;
        s_c[0][k / kApron][k % kApron] = radiance[3 * j];
        s_c[1][k / kApron][k % kApron] = radiance[3 * j + 1];
        s_c[2][k / kApron][k % kApron] = radiance[3 * j + 2];
    }
    __syncthreads();
    if (x >= W || y >= H) return;
    const size_t i = (size_t)y * (size_t)W + (size_t)x;
    const float cr = s_c[0][ty + 1][tx + 1], cg = s_c[1][ty + 1][tx + 1], cb = s_c[2][ty + 1][tx + 1];
    // motion m and the history position h = (x, y) + m
    float mx, my;
    bool valid = taa_motion(a, position, ids, x, y, i, mx, my);
    const float hx = (float)x + mx, hy = (float)y + my;
    valid = valid && hx >= 0.f && hx <= (float)(W - 1) && hy >= 0.f && hy <= (float)(H - 1);
    float len = 1.f, orr = cr, og = cg, ob = cb;
    float hr = 0.f, hg = 0.f, hb = 0.f;
    if (valid) valid = taa_resample(a, hx, hy, hr, hg, hb); // (a resampled history that is not finite is no history: ff_api.h)
    if (valid) {
        const float len_h = taa_history_length(a, hx, hy);
        if (a.clamp) {
            TaaClampBox box;
#pragma unroll
            for (int dy = 0; dy < 3; ++dy) {
#pragma unroll
                for (int dx = 0; dx < 3; ++dx) box.add(s_c[0][ty + dy][tx + dx], s_c[1][ty + dy][tx + dx], s_c[2][ty + dy][tx + dx]);
            }
            box.clamp(a.gamma, hr, hg, hb);
        }
        len = fminf(len_h + 1.f, kTaaMaxLength);
        const float alpha = fmaxf(a.alpha_min, 1.f / len);
        orr = hr + alpha * (cr - hr);
        og = hg + alpha * (cg - hg);
        ob = hb + alpha * (cb - hb);
    }
    a.hist[a.cur][i] = make_float4(orr, og, ob, len);
    a.motion[i] = make_float2(mx, my);
    if (radiance_out) {
        radiance_out[3 * i] = orr;
        radiance_out[3 * i + 1] = og;
        radiance_out[3 * i + 2] = ob;
    }
    if (rgb8) {
        rgb8[3 * i] = pixel_u8(orr);
        rgb8[3 * i + 1] = pixel_u8(og);
        rgb8[3 * i + 2] = pixel_u8(ob);
    }
}

__global__ __launch_bounds__(256) void taa_history_kernel(const TaaArgs a, float* __restrict__ motion, float* __restrict__ length)
{
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    if (x >= a.width || y >= a.height) return;
    const size_t i = (size_t)y * (size_t)a.width + (size_t)x;
    if (motion) {
        const float2 m = a.motion[i];
        motion[2 * i] = m.x;
        motion[2 * i + 1] = m.y;
    }
    if (length) length[i] = a.hist[a.cur][i].w;
}

} // namespace

hipError_t launch_taa(const TaaArgs& a, const float* radiance, const float* position, const int* ids, unsigned char* rgb8, float* radiance_out,
                      hipStream_t stream)
{
    if (a.width <= 0 || a.height <= 0) return hipSuccess;
    const dim3 grid((unsigned)((a.width + kTile - 1) / kTile), (unsigned)((a.height + kTile - 1) / kTile));
    hipLaunchKernelGGL(taa_kernel, grid, dim3(kTile * kTile), 0, stream, a, radiance, position, ids, rgb8, radiance_out);
    return hipGetLastError();
}

hipError_t launch_taa_history(const TaaArgs& a, float* motion, float* length, hipStream_t stream)
{
    if (a.width <= 0 || a.height <= 0) return hipSuccess;
    const dim3 grid((unsigned)((a.width + 63) / 64), (unsigned)((a.height + 3) / 4));
    hipLaunchKernelGGL(taa_history_kernel, grid, dim3(64, 4), 0, stream, a, motion, length);
    return hipGetLastError();
}

} // namespace ff
