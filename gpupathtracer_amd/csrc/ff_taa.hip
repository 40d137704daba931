// ff_taa.hip — the temporal anti-aliasing resolve behind ff_taa (Karis 2014, Salvi 2016).  A translation unit of its own beside
// ff_denoise.hip, ff_temporal.hip and the trace kernels, which it does not touch.  The formulas are
// in include/firefly/ff_api.h.
//
// One launch per call: 16x16-pixel workgroups.  The workgroup's 18x18 tile of radiance (its one-pixel apron clamped at the image
// borders) is staged in LDS for the 3x3 clamp statistics; the history taps are float4 loads {rgb, len} from the buffer the
// previous call wrote.  No atomics, no cross-workgroup waits: every output is a function of the inputs and the history alone.
#include "ff_taa.h"

namespace ff {
namespace {

constexpr int kTile = 16;
constexpr int kApron = kTile + 2;
constexpr float kMaxLength = 4096.f;

__device__ __forceinline__ unsigned char to_u8(float v)
{
    // the project's 8-bit rule (kernel.cu:214 truncation, out-of-range values clamped): ff_kernels.hip to_u8
    const float s = v * 255.0f;
    if (!(s > 0.0f)) return 0;
    if (s >= 255.0f) return 255;
    return (unsigned char)s;
}

// P(M, X) of ff_api.h: q = inverse(M) (X, 1); false when q.w <= 0 (or NaN)
__device__ __forceinline__ bool project(const float* P, float x, float y, float z, float sw, float sh, float& fx, float& fy)
{
    const float qx = (P[0] * x + P[4] * y) + (P[8] * z + P[12]);
    const float qy = (P[1] * x + P[5] * y) + (P[9] * z + P[13]);
    const float qw = (P[3] * x + P[7] * y) + (P[11] * z + P[15]);
    if (!(qw > 0.f)) return false;
    fx = (qx / qw + 1.f) * 0.5f * sw;
    fy = (1.f - qy / qw) * 0.5f * sh;
    return true;
}

// Catmull-Rom weights of taps -1 .. 2 for fraction t (not renormalised; they sum to 1 up to rounding)
__device__ __forceinline__ void catmull_rom(float t, float* w)
{
    const float t2 = t * t, t3 = t2 * t;
    w[0] = ((-t3 + 2.f * t2) - t) * 0.5f;
    w[1] = ((3.f * t3 - 5.f * t2) + 2.f) * 0.5f;
    w[2] = ((-3.f * t3 + 4.f * t2) + t) * 0.5f;
    w[3] = (t3 - t2) * 0.5f;
}

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
    float mx = 0.f, my = 0.f;
    bool valid = false;
    if (a.has_history) {
        const int geom = ids[3 * i];
        const bool hit = geom >= 0;
        int gflags = 0;
        bool known = true;
        if (hit) {
            if (geom < a.num_geoms) gflags = __float_as_int(a.geoms[geom].n[0].w);
            else known = false;
        }
        const bool moved = (gflags & kTpMoved) != 0;
        if (known && a.cam_rest && !moved) {
            valid = true; // (m = 0 exactly: nothing is projected)
        } else if (known) {
            float Xx, Xy, Xz, bx, by;
            bool base = true;
            if (hit) {
                const float px = position[3 * i], py = position[3 * i + 1], pz = position[3 * i + 2];
                Xx = px;
                Xy = py;
                Xz = pz;
                if (moved) {
                    const TemporalGeom& G = a.geoms[geom];
                    Xx = (G.a[0].x * px + G.a[0].y * py) + (G.a[0].z * pz + G.a[0].w);
                    Xy = (G.a[1].x * px + G.a[1].y * py) + (G.a[1].z * pz + G.a[1].w);
                    Xz = (G.a[2].x * px + G.a[2].y * py) + (G.a[2].z * pz + G.a[2].w);
                }
                base = project(a.inv_cur, px, py, pz, a.screen_w, a.screen_h, bx, by); // ~ (x + jx, y + jy)
            } else {
                // kernel.cu:200-203 for the unjittered pixel corner: the far point of the ray
                const float Px = ((float)x / a.screen_w) * 2.f - 1.f, Py = 1.f - ((float)y / a.screen_h) * 2.f;
                const float v0 = Px * a.far_clip, v1 = Py * a.far_clip, v2 = 1.f * a.far_clip, v3 = 1.f * a.far_clip;
                const float* M = a.ray;
                Xx = (M[0] * v0 + M[4] * v1) + (M[8] * v2 + M[12] * v3);
                Xy = (M[1] * v0 + M[5] * v1) + (M[9] * v2 + M[13] * v3);
                Xz = (M[2] * v0 + M[6] * v1) + (M[10] * v2 + M[14] * v3);
                bx = (float)x;
                by = (float)y;
            }
            float fx, fy;
            if (base && project(a.inv_prev, Xx, Xy, Xz, a.prev_screen_w, a.prev_screen_h, fx, fy)) {
                mx = fx - bx;
                my = fy - by;
                valid = true;
            }
        }
        if (gflags & kTpReplaced) valid = false;
    }
    const float hx = (float)x + mx, hy = (float)y + my;
    valid = valid && hx >= 0.f && hx <= (float)(W - 1) && hy >= 0.f && hy <= (float)(H - 1);
    float len = 1.f, orr = cr, og = cg, ob = cb;
    float hr = 0.f, hg = 0.f, hb = 0.f;
    if (valid) {
        const float4* __restrict__ prev = a.hist[1 - a.cur];
        const float flx = floorf(hx), fly = floorf(hy);
        const int x0 = (int)flx, y0 = (int)fly;
        const float ttx = hx - flx, tty = hy - fly;
        if (a.bilinear) {
            const float wx[2] = { 1.f - ttx, ttx }, wy[2] = { 1.f - tty, tty };
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                const size_t row = (size_t)min(y0 + r, H - 1) * (size_t)W;
#pragma unroll
                for (int c = 0; c < 2; ++c) {
                    const float4 v = prev[row + (size_t)min(x0 + c, W - 1)];
                    const float w = wy[r] * wx[c];
                    hr += w * v.x;
                    hg += w * v.y;
                    hb += w * v.z;
                }
            }
        } else {
            float wx[4], wy[4];
            catmull_rom(ttx, wx);
            catmull_rom(tty, wy);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const size_t row = (size_t)min(max(y0 - 1 + r, 0), H - 1) * (size_t)W;
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const float4 v = prev[row + (size_t)min(max(x0 - 1 + c, 0), W - 1)];
                    const float w = wy[r] * wx[c];
                    hr += w * v.x;
                    hg += w * v.y;
                    hb += w * v.z;
                }
            }
        }
        // a resampled history that is not finite is no history (ff_api.h): a NaN or Inf stored by an earlier call would otherwise
        // stay (Catmull-Rom's zero weights at rest multiply it: 0 * NaN = NaN) or turn into the clamp box's bound
        valid = isfinite(hr) && isfinite(hg) && isfinite(hb);
    }
    if (valid) {
        const int nx = min((int)floorf(hx + 0.5f), W - 1), ny = min((int)floorf(hy + 0.5f), H - 1);
        const float len_h = a.hist[1 - a.cur][(size_t)ny * (size_t)W + (size_t)nx].w;
        if (a.clamp) {
            // the 3x3 neighbourhood of the current frame in YCoCg: mean, standard deviation, min and max per channel over its n
            // finite samples (a NaN or Inf sample would make every neighbour's box, and so its output, non-finite)
            float s1[3] = { 0.f, 0.f, 0.f }, s2[3] = { 0.f, 0.f, 0.f };
            float lo[3] = { INFINITY, INFINITY, INFINITY }, hi[3] = { -INFINITY, -INFINITY, -INFINITY };
            int n = 0;
#pragma unroll
            for (int dy = 0; dy < 3; ++dy) {
#pragma unroll
                for (int dx = 0; dx < 3; ++dx) {
                    const float r = s_c[0][ty + dy][tx + dx], g = s_c[1][ty + dy][tx + dx], b = s_c[2][ty + dy][tx + dx];
                    if (!(isfinite(r) && isfinite(g) && isfinite(b))) continue;
                    ++n;
                    const float q[3] = { (0.25f * r + 0.5f * g) + 0.25f * b, 0.5f * r - 0.5f * b, (-0.25f * r + 0.5f * g) - 0.25f * b };
#pragma unroll
                    for (int ch = 0; ch < 3; ++ch) {
                        s1[ch] += q[ch];
                        s2[ch] += q[ch] * q[ch];
                        lo[ch] = fminf(lo[ch], q[ch]);
                        hi[ch] = fmaxf(hi[ch], q[ch]);
                    }
                }
            }
            const float inv_n = n == 9 ? 1.f / 9.f : 1.f / (float)n; // (all nine finite: the constant, as before)
            float h[3] = { (0.25f * hr + 0.5f * hg) + 0.25f * hb, 0.5f * hr - 0.5f * hb, (-0.25f * hr + 0.5f * hg) - 0.25f * hb };
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                const float mu = s1[ch] * inv_n;
                const float sigma = sqrtf(fmaxf(0.f, s2[ch] * inv_n - mu * mu));
                const float bl = fmaxf(lo[ch], mu - a.gamma * sigma), bh = fminf(hi[ch], mu + a.gamma * sigma);
                h[ch] = fminf(fmaxf(h[ch], bl), bh);
            }
            hr = (h[0] + h[1]) - h[2];
            hg = h[0] + h[2];
            hb = (h[0] - h[1]) - h[2];
        }
        len = fminf(len_h + 1.f, kMaxLength);
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
        rgb8[3 * i] = to_u8(orr);
        rgb8[3 * i + 1] = to_u8(og);
        rgb8[3 * i + 2] = to_u8(ob);
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
