// ff_taa_common.h — the device code ff_taa.hip and ff_taa_upscale.hip share: the motion of a pixel through the G-buffer, the
// resampling of the {rgb, len} history (Catmull-Rom or bilinear) and the YCoCg clamp box.  Every function is __forceinline__ and
// keeps the operation order ff_taa.hip had when the code lived there, so the bits of ff_taa are what they were (the library is
// built with -ffp-contract=off and without fast-math: an expression's value is fixed by its parentheses).  The formulas are in
// include/firefly/ff_api.h.  Device code only: include it from a .hip file.
#pragma once

#include "ff_pixel.h"
#include "ff_taa.h"

namespace ff {

constexpr float kTaaMaxLength = 4096.f;

// P(M, X) of ff_api.h is taa_project in ff_pixel.h (host and device: ff_interpolate.h projects with the same body).

// Catmull-Rom weights of taps -1 .. 2 for fraction t (not renormalised; they sum to 1 up to rounding)
__device__ __forceinline__ void taa_catmull_rom(float t, float* w)
{
    const float t2 = t * t, t3 = t2 * t;
    w[0] = ((-t3 + 2.f * t2) - t) * 0.5f;
    w[1] = ((3.f * t3 - 5.f * t2) + 2.f) * 0.5f;
    w[2] = ((-3.f * t3 + 4.f * t2) + t) * 0.5f;
    w[3] = (t3 - t2) * 0.5f;
}

// "motion" of ff_api.h for pixel (x, y), index i, of the a.width x a.height grid: m into (mx, my), 0 where nothing is projected.
// Returns whether the history is valid so far (there is one, q.w > 0, the mesh was not replaced); the caller bounds h.
__device__ __forceinline__ bool taa_motion(const TaaArgs& a, const float* __restrict__ position, const int* __restrict__ ids, int x, int y, size_t i,
                                           float& mx, float& my)
{
    mx = 0.f;
    my = 0.f;
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
                base = taa_project(a.inv_cur, px, py, pz, a.screen_w, a.screen_h, bx, by); // ~ (x + jx, y + jy)
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
            if (base && taa_project(a.inv_prev, Xx, Xy, Xz, a.prev_screen_w, a.prev_screen_h, fx, fy)) {
                mx = fx - bx;
                my = fy - by;
                valid = true;
            }
        }
        if (gflags & kTpReplaced) valid = false;
    }
    return valid;
}

// "history" of ff_api.h: the colour of the previous call's history at (hx, hy), which lies inside the image.  False when it is not
// finite: a NaN or Inf stored by an earlier call would otherwise stay (Catmull-Rom's zero weights at rest multiply it:
// 0 * NaN = NaN) or turn into the clamp box's bound.
__device__ __forceinline__ bool taa_resample(const TaaArgs& a, float hx, float hy, float& hr, float& hg, float& hb)
{
    const int W = a.width, H = a.height;
    hr = 0.f;
    hg = 0.f;
    hb = 0.f;
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
        taa_catmull_rom(ttx, wx);
        taa_catmull_rom(tty, wy);
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
    return isfinite(hr) && isfinite(hg) && isfinite(hb);
}

// len_h: the history length at the nearest tap floor(h + 0.5)
__device__ __forceinline__ float taa_history_length(const TaaArgs& a, float hx, float hy)
{
    const int nx = min((int)floorf(hx + 0.5f), a.width - 1), ny = min((int)floorf(hy + 0.5f), a.height - 1);
    return a.hist[1 - a.cur][(size_t)ny * (size_t)a.width + (size_t)nx].w;
}

// "clamp" of ff_api.h: the neighbourhood of the current frame in YCoCg: mean, standard deviation, min and max per channel over its
// n finite samples (a NaN or Inf sample would make every neighbour's box, and so its output, non-finite).  add() the nine samples
// row by row, then clamp() the history.
struct TaaClampBox {
    float s1[3] = { 0.f, 0.f, 0.f }, s2[3] = { 0.f, 0.f, 0.f };
    float lo[3] = { INFINITY, INFINITY, INFINITY }, hi[3] = { -INFINITY, -INFINITY, -INFINITY };
    int n = 0;
    __device__ __forceinline__ void add(float r, float g, float b)
    {
        if (!(isfinite(r) && isfinite(g) && isfinite(b))) return;
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
    __device__ __forceinline__ void clamp(float gamma, float& hr, float& hg, float& hb) const
    {
        const float inv_n = n == 9 ? 1.f / 9.f : 1.f / (float)n; // (all nine finite: the constant, as before)
        float h[3] = { (0.25f * hr + 0.5f * hg) + 0.25f * hb, 0.5f * hr - 0.5f * hb, (-0.25f * hr + 0.5f * hg) - 0.25f * hb };
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            const float mu = s1[ch] * inv_n;
            const float sigma = sqrtf(fmaxf(0.f, s2[ch] * inv_n - mu * mu));
            const float bl = fmaxf(lo[ch], mu - gamma * sigma), bh = fminf(hi[ch], mu + gamma * sigma);
            h[ch] = fminf(fmaxf(h[ch], bl), bh);
        }
        hr = (h[0] + h[1]) - h[2];
        hg = h[0] + h[2];
        hb = (h[0] - h[1]) - h[2];
    }
};

} // namespace ff
