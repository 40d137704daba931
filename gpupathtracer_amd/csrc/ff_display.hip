// ff_display.hip — the display transform behind ff_display: W x H float3 radiance -> the uchar3 buffer a viewer uploads.  A
// translation unit of its own beside the three image filters and the trace kernels, which it does not touch (DESIGN.md section 8
// row 10).  The formulas are in include/firefly/ff_api.h.
//
//   display_histogram_kernel   luminance histogram for the automatic exposure: a grid-stride pass, one 256-bin histogram per wave
//                              in LDS, one global integer add per workgroup and non-empty bin
//   bloom_bright_down_kernel   bright pass fused with the first 2x2 reduction;  bloom_down_kernel / bloom_up_kernel: the pyramid
//   display_kernel             exposure, the last bloom tap, tone curve and encoding: one thread per four pixels (three 16-byte loads,
//                              one 12-byte store of the bytes, three 16-byte stores of the curve's output)
//
// Nothing here depends on the order of floating-point adds: the histogram counts integers, every other output is a function of
// its own inputs alone.
#include "ff_display.h"

namespace ff {
namespace {

constexpr int kHistThreads = 1024;
constexpr int kHistWaves = kHistThreads / 64;
constexpr int kDisplayThreads = 256;

__device__ __forceinline__ float luminance(float r, float g, float b) { return (0.2126f * r + 0.7152f * g) + 0.0722f * b; }

__device__ __forceinline__ bool finite3(float r, float g, float b) { return isfinite(r) && isfinite(g) && isfinite(b); }

// Twelve floats (four pixels) from p: three 16-byte loads when the buffer is 16-byte aligned, scalar loads otherwise.
template <bool VEC>
__device__ __forceinline__ void load12(const float* p, float* v)
{
    if (VEC) {
        const float4* q = reinterpret_cast<const float4*>(p);
        const float4 a = q[0], b = q[1], c = q[2];
        v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
        v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
        v[8] = c.x; v[9] = c.y; v[10] = c.z; v[11] = c.w;
    } else {
#pragma unroll
        for (int k = 0; k < 12; ++k) v[k] = p[k];
    }
}

// The histogram bin of a pixel, -1 if it is not counted (a non-finite channel, or a luminance below 2^-16 or NaN)
__device__ __forceinline__ int luminance_bin(float r, float g, float b)
{
    const float l = luminance(r, g, b);
    if (!finite3(r, g, b) || !(l >= 1.52587890625e-05f)) return -1;
    return min((int)(__float_as_uint(l) >> 20) - 888, kDisplayBins - 1);
}

template <bool VEC>
__global__ __launch_bounds__(kHistThreads) void display_histogram_kernel(const float* __restrict__ radiance, size_t pixels, unsigned* __restrict__ counters)
{
    __shared__ unsigned s_h[kHistWaves][kDisplayBins];
    for (int k = threadIdx.x; k < kHistWaves * kDisplayBins; k += kHistThreads) (&s_h[0][0])[k] = 0u;
    __syncthreads();
    unsigned* mine = s_h[threadIdx.x >> 6];
    const size_t groups = pixels / 4;
    for (size_t g = (size_t)blockIdx.x * kHistThreads + threadIdx.x; g < groups; g += (size_t)gridDim.x * kHistThreads) {
        float v[12];
        load12<VEC>(radiance + 12 * g, v);
        // neighbouring pixels mostly share a bin: one LDS add per run
        int cur = -1;
        unsigned run = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int bin = luminance_bin(v[3 * k], v[3 * k + 1], v[3 * k + 2]);
            if (bin == cur) {
                ++run;
            } else {
                if (cur >= 0) atomicAdd(&mine[cur], run);
                cur = bin;
                run = 1;
            }
        }
        if (cur >= 0) atomicAdd(&mine[cur], run);
    }
    if (blockIdx.x == 0 && threadIdx.x < (unsigned)(pixels - 4 * groups)) {
        const float* p = radiance + 3 * (4 * groups + threadIdx.x);
        const int bin = luminance_bin(p[0], p[1], p[2]);
        if (bin >= 0) atomicAdd(&mine[bin], 1u);
    }
    __syncthreads();
    if (threadIdx.x < kDisplayBins) {
        unsigned sum = 0;
#pragma unroll
        for (int w = 0; w < kHistWaves; ++w) sum += s_h[w][threadIdx.x];
        if (sum) atomicAdd(&counters[threadIdx.x], sum);
    }
}

// B_0 of one input pixel: e k, k = max(le - threshold, 0) / max(le, 1e-30); a pixel with a non-finite channel is black
__device__ __forceinline__ void bright_pass(const float* __restrict__ radiance, size_t i, float E, float threshold, float* out)
{
    const float r = radiance[3 * i], g = radiance[3 * i + 1], b = radiance[3 * i + 2];
    if (!finite3(r, g, b)) {
        out[0] = out[1] = out[2] = 0.f;
        return;
    }
    const float er = r * E, eg = g * E, eb = b * E;
    const float le = luminance(er, eg, eb);
    const float k = fmaxf(le - threshold, 0.f) / fmaxf(le, 1e-30f);
    out[0] = er * k;
    out[1] = eg * k;
    out[2] = eb * k;
}

__global__ __launch_bounds__(256) void bloom_bright_down_kernel(const float* __restrict__ radiance, int W, int H, float E, float threshold, BloomLevel dst)
{
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    if (x >= dst.w || y >= dst.h) return;
    const int x0 = min(2 * x, W - 1), x1 = min(2 * x + 1, W - 1), y0 = min(2 * y, H - 1), y1 = min(2 * y + 1, H - 1);
    float b00[3], b10[3], b01[3], b11[3];
    bright_pass(radiance, (size_t)y0 * (size_t)W + (size_t)x0, E, threshold, b00);
    bright_pass(radiance, (size_t)y0 * (size_t)W + (size_t)x1, E, threshold, b10);
    bright_pass(radiance, (size_t)y1 * (size_t)W + (size_t)x0, E, threshold, b01);
    bright_pass(radiance, (size_t)y1 * (size_t)W + (size_t)x1, E, threshold, b11);
    float d[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) d[c] = ((b00[c] + b10[c]) + (b01[c] + b11[c])) * 0.25f;
    dst.texels[(size_t)y * (size_t)dst.w + (size_t)x] = make_float4(d[0], d[1], d[2], 0.f);
}

__global__ __launch_bounds__(256) void bloom_down_kernel(BloomLevel src, BloomLevel dst)
{
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    if (x >= dst.w || y >= dst.h) return;
    const int x0 = min(2 * x, src.w - 1), x1 = min(2 * x + 1, src.w - 1), y0 = min(2 * y, src.h - 1), y1 = min(2 * y + 1, src.h - 1);
    const float4 a = src.texels[(size_t)y0 * (size_t)src.w + (size_t)x0], b = src.texels[(size_t)y0 * (size_t)src.w + (size_t)x1];
    const float4 c = src.texels[(size_t)y1 * (size_t)src.w + (size_t)x0], d = src.texels[(size_t)y1 * (size_t)src.w + (size_t)x1];
    dst.texels[(size_t)y * (size_t)dst.w + (size_t)x] =
        make_float4(((a.x + b.x) + (c.x + d.x)) * 0.25f, ((a.y + b.y) + (c.y + d.y)) * 0.25f, ((a.z + b.z) + (c.z + d.z)) * 0.25f, 0.f);
}

// up(S)(x, y): the bilinear sample of S at ((x + 0.5) / 2 - 0.5, (y + 0.5) / 2 - 0.5), taps clamped, rows combined first
__device__ __forceinline__ void bloom_up_sample(const float4* __restrict__ S, int sw, int sh, int x, int y, float* out)
{
    const int xl = (x - 1) >> 1, yl = (y - 1) >> 1;
    const int xa = min(max(xl, 0), sw - 1), xb = min(xl + 1, sw - 1), ya = min(max(yl, 0), sh - 1), yb = min(yl + 1, sh - 1);
    const float wx0 = (x & 1) ? 0.75f : 0.25f, wx1 = (x & 1) ? 0.25f : 0.75f;
    const float wy0 = (y & 1) ? 0.75f : 0.25f, wy1 = (y & 1) ? 0.25f : 0.75f;
    const float4 s00 = S[(size_t)ya * (size_t)sw + (size_t)xa], s10 = S[(size_t)ya * (size_t)sw + (size_t)xb];
    const float4 s01 = S[(size_t)yb * (size_t)sw + (size_t)xa], s11 = S[(size_t)yb * (size_t)sw + (size_t)xb];
    out[0] = (s00.x * wx0 + s10.x * wx1) * wy0 + (s01.x * wx0 + s11.x * wx1) * wy1;
    out[1] = (s00.y * wx0 + s10.y * wx1) * wy0 + (s01.y * wx0 + s11.y * wx1) * wy1;
    out[2] = (s00.z * wx0 + s10.z * wx1) * wy0 + (s01.z * wx0 + s11.z * wx1) * wy1;
}

__global__ __launch_bounds__(256) void bloom_up_kernel(BloomLevel src, BloomLevel dst)
{
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    if (x >= dst.w || y >= dst.h) return;
    float u[3];
    bloom_up_sample(src.texels, src.w, src.h, x, y, u);
    float4* t = &dst.texels[(size_t)y * (size_t)dst.w + (size_t)x];
    const float4 d = *t;
    *t = make_float4(d.x + u[0], d.y + u[1], d.z + u[2], 0.f);
}

// Steps 3 to 6 for pixel i with channels c: y[3] after the curve and its clamp, b[3] the bytes
template <int CURVE, int ENC, bool BLOOM>
__device__ __forceinline__ void display_pixel(const DisplayArgs& a, size_t i, const float* c, const float* s_t, float* y, unsigned* b)
{
    float e[3] = { c[0] * a.exposure, c[1] * a.exposure, c[2] * a.exposure };
    if (BLOOM) {
        float u[3];
        bloom_up_sample(a.u1, a.u1_w, a.u1_h, (int)(i % (size_t)a.width), (int)(i / (size_t)a.width), u);
#pragma unroll
        for (int k = 0; k < 3; ++k) e[k] = e[k] + u[k] * a.bloom_scale;
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        y[k] = display_curve<CURVE>(e[k], a.w2);
        b[k] = ENC == FF_ENCODE_SRGB ? display_srgb_u8(y[k], s_t) : display_linear_u8(y[k]);
    }
}

// radiance and display_out may be the same buffer (every thread reads its own pixels before it writes them): no __restrict__
template <int CURVE, int ENC, bool BLOOM, bool VEC>
__global__ __launch_bounds__(kDisplayThreads) void display_kernel(const DisplayArgs a, const float* radiance, unsigned char* rgb8, float* display_out)
{
    __shared__ float s_t[256];
    if (ENC == FF_ENCODE_SRGB) {
        if (threadIdx.x < kDisplayThresholds) s_t[threadIdx.x] = a.thresholds[threadIdx.x];
        __syncthreads();
    }
    const size_t pixels = (size_t)a.width * (size_t)a.height, groups = pixels / 4;
    const size_t item = (size_t)blockIdx.x * kDisplayThreads + threadIdx.x;
    if (item < groups) {
        float v[12], y[12];
        unsigned b[12];
        load12<VEC>(radiance + 12 * item, v);
#pragma unroll
        for (int k = 0; k < 4; ++k) display_pixel<CURVE, ENC, BLOOM>(a, 4 * item + k, v + 3 * k, s_t, y + 3 * k, b + 3 * k);
        if (rgb8) {
            if (VEC) {
                // twelve bytes as three words (the buffer is 4-byte aligned: the compiler makes it one 12-byte store)
                unsigned* o = reinterpret_cast<unsigned*>(rgb8 + 12 * item);
                o[0] = b[0] | b[1] << 8 | b[2] << 16 | b[3] << 24;
                o[1] = b[4] | b[5] << 8 | b[6] << 16 | b[7] << 24;
                o[2] = b[8] | b[9] << 8 | b[10] << 16 | b[11] << 24;
            } else {
#pragma unroll
                for (int k = 0; k < 12; ++k) rgb8[12 * item + k] = (unsigned char)b[k];
            }
        }
        if (display_out) {
            if (VEC) {
                float4* o = reinterpret_cast<float4*>(display_out + 12 * item);
                o[0] = make_float4(y[0], y[1], y[2], y[3]);
                o[1] = make_float4(y[4], y[5], y[6], y[7]);
                o[2] = make_float4(y[8], y[9], y[10], y[11]);
            } else {
#pragma unroll
                for (int k = 0; k < 12; ++k) display_out[12 * item + k] = y[k];
            }
        }
    } else if (item - groups < pixels - 4 * groups) {
        // the last W*H mod 4 pixels, one thread each
        const size_t i = 4 * groups + (item - groups);
        const float c[3] = { radiance[3 * i], radiance[3 * i + 1], radiance[3 * i + 2] };
        float y[3];
        unsigned b[3];
        display_pixel<CURVE, ENC, BLOOM>(a, i, c, s_t, y, b);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            if (rgb8) rgb8[3 * i + k] = (unsigned char)b[k];
            if (display_out) display_out[3 * i + k] = y[k];
        }
    }
}

template <int CURVE, int ENC, bool BLOOM>
void launch_display_vec(const DisplayArgs& a, const float* radiance, unsigned char* rgb8, float* display_out, bool vec, dim3 grid, hipStream_t stream)
{
    if (vec) hipLaunchKernelGGL((display_kernel<CURVE, ENC, BLOOM, true>), grid, dim3(kDisplayThreads), 0, stream, a, radiance, rgb8, display_out);
    else hipLaunchKernelGGL((display_kernel<CURVE, ENC, BLOOM, false>), grid, dim3(kDisplayThreads), 0, stream, a, radiance, rgb8, display_out);
}

template <int CURVE, int ENC>
void launch_display_bloom(const DisplayArgs& a, const float* radiance, unsigned char* rgb8, float* display_out, bool vec, dim3 grid, hipStream_t stream)
{
    if (a.bloom) launch_display_vec<CURVE, ENC, true>(a, radiance, rgb8, display_out, vec, grid, stream);
    else launch_display_vec<CURVE, ENC, false>(a, radiance, rgb8, display_out, vec, grid, stream);
}

template <int CURVE>
void launch_display_enc(const DisplayArgs& a, const float* radiance, unsigned char* rgb8, float* display_out, bool vec, dim3 grid, hipStream_t stream)
{
    if (a.encoding == FF_ENCODE_SRGB) launch_display_bloom<CURVE, FF_ENCODE_SRGB>(a, radiance, rgb8, display_out, vec, grid, stream);
    else launch_display_bloom<CURVE, FF_ENCODE_LINEAR>(a, radiance, rgb8, display_out, vec, grid, stream);
}

bool aligned_to(const void* p, size_t n) { return ((uintptr_t)p & (n - 1)) == 0; }

dim3 level_grid(const BloomLevel& l) { return dim3((unsigned)((l.w + 63) / 64), (unsigned)((l.h + 3) / 4)); }

} // namespace

hipError_t launch_display_histogram(const float* radiance, size_t pixels, unsigned* counters, int num_cus, hipStream_t stream)
{
    if (pixels == 0) return hipSuccess;
    // the grid follows the CU count, not the image: every workgroup adds at most 256 counters to the global ones
    const size_t want = (pixels / 4 + kHistThreads - 1) / kHistThreads;
    const unsigned grid = (unsigned)std::max<size_t>(1, std::min<size_t>(want, (size_t)std::max(num_cus, 1)));
    if (aligned_to(radiance, 16)) hipLaunchKernelGGL(display_histogram_kernel<true>, dim3(grid), dim3(kHistThreads), 0, stream, radiance, pixels, counters);
    else hipLaunchKernelGGL(display_histogram_kernel<false>, dim3(grid), dim3(kHistThreads), 0, stream, radiance, pixels, counters);
    return hipGetLastError();
}

hipError_t launch_bloom_bright_down(const float* radiance, int width, int height, float exposure, float threshold, BloomLevel dst, hipStream_t stream)
{
    hipLaunchKernelGGL(bloom_bright_down_kernel, level_grid(dst), dim3(64, 4), 0, stream, radiance, width, height, exposure, threshold, dst);
    return hipGetLastError();
}

hipError_t launch_bloom_down(BloomLevel src, BloomLevel dst, hipStream_t stream)
{
    hipLaunchKernelGGL(bloom_down_kernel, level_grid(dst), dim3(64, 4), 0, stream, src, dst);
    return hipGetLastError();
}

hipError_t launch_bloom_up(BloomLevel src, BloomLevel dst, hipStream_t stream)
{
    hipLaunchKernelGGL(bloom_up_kernel, level_grid(dst), dim3(64, 4), 0, stream, src, dst);
    return hipGetLastError();
}

hipError_t launch_display(const DisplayArgs& a, const float* radiance, unsigned char* rgb8, float* display_out, hipStream_t stream)
{
    if (a.width <= 0 || a.height <= 0) return hipSuccess;
    const size_t pixels = (size_t)a.width * (size_t)a.height, items = pixels / 4 + pixels % 4;
    const dim3 grid((unsigned)((items + kDisplayThreads - 1) / kDisplayThreads));
    const bool vec = aligned_to(radiance, 16) && aligned_to(rgb8, 4) && aligned_to(display_out, 16);
    if (a.curve == FF_CURVE_ACES) launch_display_enc<FF_CURVE_ACES>(a, radiance, rgb8, display_out, vec, grid, stream);
    else if (a.curve == FF_CURVE_REINHARD) launch_display_enc<FF_CURVE_REINHARD>(a, radiance, rgb8, display_out, vec, grid, stream);
    else launch_display_enc<FF_CURVE_CLAMP>(a, radiance, rgb8, display_out, vec, grid, stream);
    return hipGetLastError();
}

} // namespace ff
