// ff_taa_upscale.hip — the temporal upsampler behind ff_taa_upscale: ff_taa writing a larger image than it reads.  A translation
// unit of its own beside ff_taa.hip and ff_upscale.hip and the trace kernels, which it does not touch.
// The formulas are in include/firefly/ff_api.h; the motion, the history resampling and the clamp box are ff_taa's own code
// (ff_taa_common.h), the spatial estimate walks ff_upscale's taps (ff_upscale.h: upscale_taps, UpscaleMean).
//
// One launch per call over the high grid: 16x16-pixel workgroups, as in taa_kernel.  High pixel X looks at low coordinate
// u = X w / W - jx, which is monotone in X, so the low pixels a workgroup can name - the 3x3 box about the nearest sample and the
// 2x2 / 4x4 taps about floor(u) - lie in [floor(u(X0)) - 1, floor(u(X1)) + 2] per axis, X0 and X1 the tile's first and last pixel:
// at most 16 w / W + 4 <= 20 a side.  That footprint (radiance and the geometry / bxdf ids, each coordinate clamped into the low
// image) is staged in LDS: 8 000 bytes.  A tap outside the staged window - there is none, but the bound is rounding's, not the
// compiler's - is read from memory at its clamped coordinate, so no index leaves the LDS arrays or the images whatever u is.
// The history taps are float4 loads {rgb, len} from the buffer the previous call wrote, stores likewise.  No atomics, no
// cross-workgroup waits: every output is a function of the inputs and the history alone.
#include "ff_taa_common.h"
#include "ff_taa_upscale.h"
#include "ff_upscale.h"

namespace ff {
namespace {

constexpr int kTile = 16;
constexpr int kSide = kTile + 4;

// step 2: the low image coordinate high pixel X looks along
__device__ __forceinline__ float look(int X, int w, int W, float j) { return ((float)X * (float)w) / (float)W - j; }

__global__ __launch_bounds__(256) void taa_upscale_kernel(const TaaUpscaleArgs a, const float* __restrict__ radiance_lo, const int* __restrict__ ids_lo,
                                                          const float* __restrict__ position, const int* __restrict__ ids,
                                                          unsigned char* __restrict__ rgb8, float* __restrict__ radiance_out)
{
    __shared__ float s_c[3][kSide][kSide];
    __shared__ int s_g[2][kSide][kSide];
    const TaaArgs& t = a.taa;
    const int W = t.width, H = t.height, w = a.lo_width, h = a.lo_height;
    const int tx = threadIdx.x & (kTile - 1), ty = threadIdx.x / kTile;
    const int x = blockIdx.x * kTile + tx, y = blockIdx.y * kTile + ty;
    // the tile's low footprint: columns ox .. ox + nx - 1, rows oy .. oy + ny - 1 (before clamping into the image)
    const int X0 = blockIdx.x * kTile, Y0 = blockIdx.y * kTile;
    const int ox = (int)floorf(look(X0, w, W, a.lo_jx)) - 1, oy = (int)floorf(look(Y0, h, H, a.lo_jy)) - 1;
    const int nx = min((int)floorf(look(min(X0 + kTile - 1, W - 1), w, W, a.lo_jx)) + 2 - ox + 1, kSide);
    const int ny = min((int)floorf(look(min(Y0 + kTile - 1, H - 1), h, H, a.lo_jy)) + 2 - oy + 1, kSide);
    for (int k = threadIdx.x; k < nx * ny; k += kTile * kTile) {
        const int e = k % nx, f = k / nx;
        const size_t j = (size_t)upscale_clamp(oy + f, h - 1) * (size_t)w + (size_t)upscale_clamp(ox + e, w - 1);
        s_c[0][f][e] = radiance_lo[3 * j];
        s_c[1][f][e] = radiance_lo[3 * j + 1];
        s_c[2][f][e] = radiance_lo[3 * j + 2];
        s_g[0][f][e] = ids_lo[3 * j];
        s_g[1][f][e] = ids_lo[3 * j + 2];
    }
    __syncthreads();
    if (x >= W || y >= H) return;
    const size_t i = (size_t)y * (size_t)W + (size_t)x;
    // low pixel (ic, jc), both inside the image: its radiance, geometry index and bxdf type
    auto low = [&](int ic, int jc, float* c, int& geom, int& kind) {
        const int e = ic - ox, f = jc - oy;
        if ((unsigned)e < (unsigned)nx && (unsigned)f < (unsigned)ny) {
            c[0] = s_c[0][f][e];
            c[1] = s_c[1][f][e];
            c[2] = s_c[2][f][e];
            geom = s_g[0][f][e];
            kind = s_g[1][f][e];
        } else {
            const size_t j = (size_t)jc * (size_t)w + (size_t)ic;
            c[0] = radiance_lo[3 * j];
            c[1] = radiance_lo[3 * j + 1];
            c[2] = radiance_lo[3 * j + 2];
            geom = ids_lo[3 * j];
            kind = ids_lo[3 * j + 2];
        }
    };
    const int gP = ids[3 * i], kP = ids[3 * i + 2];
    // 1. motion m, the history at h = (x, y) + m and its length
    float mx, my;
    bool valid = taa_motion(t, position, ids, x, y, i, mx, my);
    const float hx = (float)x + mx, hy = (float)y + my;
    valid = valid && hx >= 0.f && hx <= (float)(W - 1) && hy >= 0.f && hy <= (float)(H - 1);
    float hr = 0.f, hg = 0.f, hb = 0.f, len_h = 0.f;
    if (valid) valid = taa_resample(t, hx, hy, hr, hg, hb);
    if (valid) len_h = taa_history_length(t, hx, hy);
    // 2. where the pixel looks in the low frame, and the nearest low sample q*
    const float u = look(x, w, W, a.lo_jx), v = look(y, h, H, a.lo_jy);
    const int is = upscale_clamp((int)floorf(u + 0.5f), w - 1), js = upscale_clamp((int)floorf(v + 0.5f), h - 1);
    const float dx = u - (float)is, dy = v - (float)js;
    // 3. confidence: a tent one high pixel wide about the point the low ray went through; 0 for another surface or a bad sample
    float k = fmaxf(0.f, 1.f - fabsf(dx) * a.sx) * fmaxf(0.f, 1.f - fabsf(dy) * a.sy);
    float c[3];
    int gq, kq;
    low(is, js, c, gq, kq);
    if (gq != gP || kq != kP) k = 0.f;
    if (!(pixel_finite(c[0]) && pixel_finite(c[1]) && pixel_finite(c[2]))) k = 0.f;
    // 6. blend (5, the clamp, inside its first case)
    float o[3], len;
    const float wsum = valid ? fminf(len_h + k, kTaaMaxLength) : 0.f;
    if (valid && wsum > 0.f && k > 0.f) {
        if (t.clamp) {
            TaaClampBox box;
#pragma unroll
            for (int r = -1; r <= 1; ++r) {
#pragma unroll
                for (int s = -1; s <= 1; ++s) {
                    float n[3];
                    int gn, kn;
                    low(upscale_clamp(is + s, w - 1), upscale_clamp(js + r, h - 1), n, gn, kn);
                    box.add(n[0], n[1], n[2]);
                }
            }
            if (box.n > 0) box.clamp(t.gamma, hr, hg, hb);
        }
        const float alpha = fmaxf(t.alpha_min * k, k / wsum);
        o[0] = hr + alpha * (c[0] - hr);
        o[1] = hg + alpha * (c[1] - hg);
        o[2] = hb + alpha * (c[2] - hb);
        len = wsum;
    } else if (valid && wsum > 0.f) {
        o[0] = hr; // (the history as it is: no sample for this pixel in this frame)
        o[1] = hg;
        o[2] = hb;
        len = len_h;
    } else if (!valid && k > 0.f) {
        o[0] = c[0];
        o[1] = c[1];
        o[2] = c[2];
        len = k;
    } else {
        // 4. nothing of the pixel's own, now or before: the spatial estimate c_up (ff_upscale's step 3 for every P, then its step 4)
        UpscaleArgs ua;
        ua.lo_width = w;
        ua.lo_height = h;
        const float flu = floorf(u), flv = floorf(v);
        UpscaleMean m;
        const bool any = upscale_taps(ua, (int)flu, (int)flv, u - flu, v - flv, [&](size_t q, float b) {
            const unsigned jc = (unsigned)q / (unsigned)w, ic = (unsigned)q - jc * (unsigned)w; // (w h < 2^32)
            float n[3];
            int gn, kn;
            low((int)ic, (int)jc, n, gn, kn);
            if (gn != gP || kn != kP) return false;
            if (!(pixel_finite(n[0]) && pixel_finite(n[1]) && pixel_finite(n[2]))) return false;
            m.add(b, n[0], n[1], n[2]);
            return true;
        });
        if (any) {
            m.get(o);
        } else {
            o[0] = c[0]; // (the nearest low pixel q* as it is)
            o[1] = c[1];
            o[2] = c[2];
        }
        len = 0.f;
    }
    t.hist[t.cur][i] = make_float4(o[0], o[1], o[2], len);
    t.motion[i] = make_float2(mx, my);
    if (radiance_out) {
        radiance_out[3 * i] = o[0];
        radiance_out[3 * i + 1] = o[1];
        radiance_out[3 * i + 2] = o[2];
    }
    if (rgb8) {
        rgb8[3 * i] = pixel_u8(o[0]);
        rgb8[3 * i + 1] = pixel_u8(o[1]);
        rgb8[3 * i + 2] = pixel_u8(o[2]);
    }
}

} // namespace

hipError_t launch_taa_upscale(const TaaUpscaleArgs& a, const float* radiance_lo, const int* ids_lo, const float* position, const int* ids,
                              unsigned char* rgb8, float* radiance_out, hipStream_t stream)
{
    if (a.taa.width <= 0 || a.taa.height <= 0 || a.lo_width <= 0 || a.lo_height <= 0) return hipSuccess;
    const dim3 grid((unsigned)((a.taa.width + kTile - 1) / kTile), (unsigned)((a.taa.height + kTile - 1) / kTile));
    hipLaunchKernelGGL(taa_upscale_kernel, grid, dim3(kTile * kTile), 0, stream, a, radiance_lo, ids_lo, position, ids, rgb8, radiance_out);
    return hipGetLastError();
}

} // namespace ff
