// ff_temporal.hip — the temporal denoiser behind ff_denoise_temporal: spatiotemporal variance-guided filtering (SVGF, Schied et al.
// 2017) on the G-buffer of ff_gbuffer.  A translation unit of its own beside ff_denoise.hip and the trace kernels, which it does not
// touch; the output step is ff_denoise.hip's finish kernel.  The formulas are in include/firefly/ff_api.h.
//
// Four steps per call: reproject + accumulate (one thread per pixel, rows of 64 pixels per wave), the 7x7 spatial variance of
// pixels with a short history, the variance-guided à-trous passes (16x16-pixel workgroups, one launch per pass, ping-pong buffers)
// and the finish.  No atomics, no cross-workgroup waits: every output is a function of the inputs and the history alone.
#include "ff_temporal.h"

namespace ff {
namespace {

__device__ __forceinline__ float dot3(float ax, float ay, float az, float bx, float by, float bz)
{
    const float px = ax * bx, py = ay * by, pz = az * bz;
    return (px + py) + pz;
}

__device__ __forceinline__ float luminance(float r, float g, float b) { return (0.2126f * r + 0.7152f * g) + 0.0722f * b; }

__device__ __forceinline__ bool finite3(float a, float b, float c) { return isfinite(a) && isfinite(b) && isfinite(c); }

constexpr int kTile = 16;            // pass workgroups: 16 x 16 pixels, as ff_denoise's
constexpr float kPlaneEps = 1e-30f;  // as ff_denoise: |x_q - x_p|^2 = 0 for coincident points
constexpr float kLumEps = 1e-30f;    // keeps sigma_l sqrt(g) = 0 finite
constexpr float kMaxExponent = 30.f; // as ff_denoise: taps with an exponent above 30 weigh 0
constexpr float kMinHistoryWeight = 1e-3f; // summed bilinear weight of the valid taps below which a pixel starts afresh
__constant__ float kB3[5] = { 1.f / 16.f, 1.f / 4.f, 3.f / 8.f, 1.f / 4.f, 1.f / 16.f };

__global__ __launch_bounds__(256) void temporal_reproject_kernel(const TemporalBuffers b, const TemporalReproject r, const float* __restrict__ radiance,
                                                                 const float* __restrict__ position, const float* __restrict__ normal,
                                                                 const float* __restrict__ albedo, const int* __restrict__ ids)
{
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    const int W = b.width, H = b.height;
    if (x >= W || y >= H) return;
    const size_t i = (size_t)y * (size_t)W + (size_t)x;
    const int cur = r.cur, prev = 1 - r.cur;
    // this call's guides: ff_denoise's pack
    const int geom = ids[3 * i], bxdf = ids[3 * i + 2];
    const bool filt = geom >= 0 && bxdf != FF_BXDF_EMITTER && bxdf != FF_BXDF_MIRROR && bxdf != FF_BXDF_GLASS;
    const int cls = filt ? geom : -1;
    float nx = normal[3 * i], ny = normal[3 * i + 1], nz = normal[3 * i + 2];
    const float n2 = dot3(nx, ny, nz, nx, ny, nz);
    const float inv = n2 > 0.f ? 1.0f / sqrtf(n2) : 0.f;
    nx *= inv;
    ny *= inv;
    nz *= inv;
    const float px = position[3 * i], py = position[3 * i + 1], pz = position[3 * i + 2];
    b.pos[cur][i] = make_float4(px, py, pz, __int_as_float(cls));
    b.nrm[cur][i] = make_float4(nx, ny, nz, 0.f);
    float cx = radiance[3 * i], cy = radiance[3 * i + 1], cz = radiance[3 * i + 2];
    if (r.demodulate && filt) {
        const float ax = albedo[3 * i], ay = albedo[3 * i + 1], az = albedo[3 * i + 2];
        if (ax > 0.f) cx = cx / ax;
        if (ay > 0.f) cy = cy / ay;
        if (az > 0.f) cz = cz / az;
    }
    const float l = luminance(cx, cy, cz);
    float mx = 0.f, my = 0.f;
    float wsum = 0.f, hx = 0.f, hy = 0.f, hz = 0.f, h1 = 0.f, h2 = 0.f, hl = 0.f;
    if (r.has_history && geom >= 0 && geom < r.num_geoms) {
        const TemporalGeom& G = r.geoms[geom];
        const int gflags = __float_as_int(G.n[0].w);
        const bool moved = (gflags & kTpMoved) != 0;
        // x^: the point where the previous call saw this surface point
        float xh = px, yh = py, zh = pz;
        if (moved) {
            xh = (G.a[0].x * px + G.a[0].y * py) + (G.a[0].z * pz + G.a[0].w);
            yh = (G.a[1].x * px + G.a[1].y * py) + (G.a[1].z * pz + G.a[1].w);
            zh = (G.a[2].x * px + G.a[2].y * py) + (G.a[2].z * pz + G.a[2].w);
        }
        // its pixel in the previous image: inverse(ray matrix) (x^, 1), divided by w; the primary ray's mapping inverted
        float fx = (float)x, fy = (float)y;
        bool seen = true;
        if (!(r.at_rest && !moved)) {
            const float* P = r.proj;
            const float qx = (P[0] * xh + P[4] * yh) + (P[8] * zh + P[12]);
            const float qy = (P[1] * xh + P[5] * yh) + (P[9] * zh + P[13]);
            const float qw = (P[3] * xh + P[7] * yh) + (P[11] * zh + P[15]);
            seen = qw > 0.f; // (a point behind the previous camera has no pixel there)
            if (seen) {
                fx = (qx / qw + 1.f) * 0.5f * r.screen_w;
                fy = (1.f - qy / qw) * 0.5f * r.screen_h;
            }
        }
        if (seen) {
            mx = fx - (float)x;
            my = fy - (float)y;
        }
        if (seen && filt && !(gflags & kTpReplaced) && fx > -1.f && fx < (float)W && fy > -1.f && fy < (float)H) {
            float hnx = nx, hny = ny, hnz = nz;
            if (moved) {
                hnx = dot3(G.n[0].x, G.n[0].y, G.n[0].z, nx, ny, nz);
                hny = dot3(G.n[1].x, G.n[1].y, G.n[1].z, nx, ny, nz);
                hnz = dot3(G.n[2].x, G.n[2].y, G.n[2].z, nx, ny, nz);
                const float h2n = dot3(hnx, hny, hnz, hnx, hny, hnz);
                const float hinv = h2n > 0.f ? 1.0f / sqrtf(h2n) : 0.f;
                hnx *= hinv;
                hny *= hinv;
                hnz *= hinv;
            }
            const float ex = xh - r.eye[0], ey = yh - r.eye[1], ez = zh - r.eye[2];
            const float plane_lim = r.reuse_plane * sqrtf(dot3(ex, ey, ez, ex, ey, ez));
            const float flx = floorf(fx), fly = floorf(fy);
            const int x0 = (int)flx, y0 = (int)fly; // (in -1 .. W-1, -1 .. H-1 by the test above)
            const float ax = fx - flx, ay = fy - fly;
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const int tx = x0 + (t & 1), ty = y0 + (t >> 1);
                const float w = ((t & 1) ? ax : 1.f - ax) * ((t >> 1) ? ay : 1.f - ay);
                if (tx < 0 || tx >= W || ty < 0 || ty >= H || w == 0.f) continue;
                const size_t j = (size_t)ty * (size_t)W + (size_t)tx;
                const float4 gq = b.pos[prev][j];
                if (__float_as_int(gq.w) != cls) continue;
                const float4 nq = b.nrm[prev][j];
                if (!(dot3(hnx, hny, hnz, nq.x, nq.y, nq.z) >= r.reuse_normal)) continue;
                if (!(fabsf(dot3(hnx, hny, hnz, gq.x - xh, gq.y - yh, gq.z - zh)) <= plane_lim)) continue;
                const float4 cq = b.col[prev][j];
                const float4 mq = b.mom[prev][j];
                // a stored value that is not finite is no history (ff_api.h): one NaN or Inf sample would otherwise stay in the
                // blend for good at rest and spread through the bilinear taps under motion
                if (!(finite3(cq.x, cq.y, cq.z) && finite3(mq.x, mq.y, mq.z))) continue;
                wsum += w;
                hx += w * cq.x;
                hy += w * cq.y;
                hz += w * cq.z;
                h1 += w * mq.x;
                h2 += w * mq.y;
                hl += w * mq.z;
            }
        }
    }
    float len = 1.f, ox = cx, oy = cy, oz = cz, m1 = l, m2 = l * l;
    if (wsum >= kMinHistoryWeight) {
        hx = hx / wsum;
        hy = hy / wsum;
        hz = hz / wsum;
        h1 = h1 / wsum;
        h2 = h2 / wsum;
        len = hl / wsum + 1.f;
        const float alpha = 1.f / fminf(len, r.max_history);
        ox = hx + alpha * (cx - hx);
        oy = hy + alpha * (cy - hy);
        oz = hz + alpha * (cz - hz);
        m1 = h1 + alpha * (l - h1);
        m2 = h2 + alpha * (m2 - h2);
    }
    if (!filt) len = m1 = m2 = 0.f;
    const float var = (filt && len >= r.variance_history) ? fmaxf(0.f, m2 - m1 * m1) : 0.f;
    b.mom[cur][i] = make_float4(m1, m2, len, 0.f);
    b.work[0][i] = make_float4(ox, oy, oz, var);
    if (r.feedback_unfiltered) b.col[cur][i] = make_float4(ox, oy, oz, 0.f);
    b.motion[i] = make_float2(mx, my);
}

// The spatial variance of a short history: the moments averaged over 7x7 with ff_denoise's w_n w_x on the pixel's own class.
__global__ __launch_bounds__(256) void temporal_variance_kernel(const TemporalBuffers b, int cur, float variance_history, float inv_sigma_normal,
                                                                float sigma_plane2)
{
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    const int W = b.width, H = b.height;
    if (x >= W || y >= H) return;
    const size_t i = (size_t)y * (size_t)W + (size_t)x;
    const float4 gp = b.pos[cur][i];
    const int cls = __float_as_int(gp.w);
    if (cls < 0) return;
    const float4 mp = b.mom[cur][i];
    if (mp.z >= variance_history) return; // (the reprojection wrote its temporal estimate)
    const float4 np = b.nrm[cur][i];
    float wsum = 1.f, s1 = mp.x, s2 = mp.y;
    for (int dy = -3; dy <= 3; ++dy) {
        const int yy = y + dy;
        if (yy < 0 || yy >= H) continue;
        for (int dx = -3; dx <= 3; ++dx) {
            const int xx = x + dx;
            if ((dx == 0 && dy == 0) || xx < 0 || xx >= W) continue;
            const size_t j = (size_t)yy * (size_t)W + (size_t)xx;
            const float4 gq = b.pos[cur][j];
            if (__float_as_int(gq.w) != cls) continue;
            const float4 nq = b.nrm[cur][j];
            const float a_n = (1.0f - dot3(np.x, np.y, np.z, nq.x, nq.y, nq.z)) * inv_sigma_normal;
            const float vx = gq.x - gp.x, vy = gq.y - gp.y, vz = gq.z - gp.z;
            const float pd = dot3(np.x, np.y, np.z, vx, vy, vz);
            const float a_x = pd * pd * __builtin_amdgcn_rcpf(sigma_plane2 * dot3(vx, vy, vz, vx, vy, vz) + kPlaneEps);
            const float e = a_n + a_x;
            if (!(e <= kMaxExponent)) continue;
            const float w = __expf(-e);
            const float4 mq = b.mom[cur][j];
            wsum += w;
            s1 += w * mq.x;
            s2 += w * mq.y;
        }
    }
    const float mu1 = s1 / wsum, mu2 = s2 / wsum;
    float4 c = b.work[0][i];
    c.w = fmaxf(0.f, mu2 - mu1 * mu1) * 4.f / mp.z;
    b.work[0][i] = c;
}

// One variance-guided pass: ff_denoise's pass with the colour edge-stop replaced by w_l = exp(-|l_p - l_q| / (sigma_l sqrt(g_p) + eps)),
// g_p the 3x3 (1 2 1)^2 Gaussian of the variance over the taps that count; the variance follows as sum w^2 var_q / (sum w)^2.
// The classes and variances of the workgroup's tile and its one-pixel apron are staged in LDS first (18 x 18: 1.3 loads per
// thread instead of 16 for the 3x3 neighbourhood); pixels outside the image read as class -1.
__global__ __launch_bounds__(256) void temporal_pass_kernel(const TemporalBuffers b, int cur, int src, int step, float sigma_luminance,
                                                            float inv_sigma_normal, float sigma_plane2, int same_geometry, float4* __restrict__ feedback)
{
    constexpr int kApron = kTile + 2;
    __shared__ int s_cls[kApron][kApron];
    __shared__ float s_var[kApron][kApron];
    const int tx = threadIdx.x & (kTile - 1), ty = threadIdx.x / kTile;
    const int x = blockIdx.x * kTile + tx, y = blockIdx.y * kTile + ty;
    const int W = b.width, H = b.height;
    const float4* __restrict__ cin = b.work[src];
    for (int k = threadIdx.x; k < kApron * kApron; k += kTile * kTile) {
        const int gx = (int)blockIdx.x * kTile - 1 + k % kApron, gy = (int)blockIdx.y * kTile - 1 + k / kApron;
        int c = -1;
        float v = 0.f;
        if (gx >= 0 && gx < W && gy >= 0 && gy < H) {
            const size_t j = (size_t)gy * (size_t)W + (size_t)gx;
            c = __float_as_int(b.pos[cur][j].w);
            v = cin[j].w;
        }
        s_cls[k / kApron][k % kApron] = c;
        s_var[k / kApron][k % kApron] = v;
    }
    __syncthreads();
    if (x >= W || y >= H) return;
    const size_t i = (size_t)y * (size_t)W + (size_t)x;
    const float4 gp = b.pos[cur][i];
    const int cls = __float_as_int(gp.w);
    if (cls < 0) return;
    const float4 np = b.nrm[cur][i];
    const float4 cp = cin[i];
    float ksum = 4.f, gsum = 4.f * cp.w;
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy) {
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx) {
            if (dx == 0 && dy == 0) continue;
            const int qcls = s_cls[ty + 1 + dy][tx + 1 + dx];
            if (qcls < 0 || (same_geometry && qcls != cls)) continue;
            const float k = (float)((2 - (dx < 0 ? -dx : dx)) * (2 - (dy < 0 ? -dy : dy)));
            ksum += k;
            gsum += k * s_var[ty + 1 + dy][tx + 1 + dx];
        }
    }
    const float lp = luminance(cp.x, cp.y, cp.z);
    const float lcoef = __builtin_amdgcn_rcpf(sigma_luminance * sqrtf(gsum / ksum) + kLumEps);
    const float h0 = kB3[2] * kB3[2];
    float wsum = h0, vsum = h0 * h0 * cp.w, sx = 0.f, sy = 0.f, sz = 0.f;
#pragma unroll
    for (int dy = -2; dy <= 2; ++dy) {
        const int yy = y + dy * step;
        if (yy < 0 || yy >= H) continue;
#pragma unroll
        for (int dx = -2; dx <= 2; ++dx) {
            if (dx == 0 && dy == 0) continue;
            const int xx = x + dx * step;
            if (xx < 0 || xx >= W) continue;
            const size_t j = (size_t)yy * (size_t)W + (size_t)xx;
            const float4 gq = b.pos[cur][j];
            const int qcls = __float_as_int(gq.w);
            if (qcls < 0 || (same_geometry && qcls != cls)) continue;
            const float4 nq = b.nrm[cur][j];
            const float4 cq = cin[j];
            const float a_l = fabsf(lp - luminance(cq.x, cq.y, cq.z)) * lcoef;
            const float a_n = (1.0f - dot3(np.x, np.y, np.z, nq.x, nq.y, nq.z)) * inv_sigma_normal;
            const float vx = gq.x - gp.x, vy = gq.y - gp.y, vz = gq.z - gp.z;
            const float pd = dot3(np.x, np.y, np.z, vx, vy, vz);
            const float a_x = pd * pd * __builtin_amdgcn_rcpf(sigma_plane2 * dot3(vx, vy, vz, vx, vy, vz) + kPlaneEps);
            const float e = a_l + a_n + a_x;
            if (!(e <= kMaxExponent)) continue;
            const float w = (kB3[dx + 2] * kB3[dy + 2]) * __expf(-e);
            wsum += w;
            vsum += (w * w) * cq.w;
            sx += w * (cp.x - cq.x);
            sy += w * (cp.y - cq.y);
            sz += w * (cp.z - cq.z);
        }
    }
    const float rw = __builtin_amdgcn_rcpf(wsum);
    const float4 out = make_float4(cp.x - sx * rw, cp.y - sy * rw, cp.z - sz * rw, vsum * rw * rw);
    b.work[1 - src][i] = out;
    if (feedback) feedback[i] = make_float4(out.x, out.y, out.z, 0.f);
}

__global__ __launch_bounds__(256) void temporal_history_kernel(const TemporalBuffers b, int cur, float* __restrict__ motion, float* __restrict__ length)
{
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    if (x >= b.width || y >= b.height) return;
    const size_t i = (size_t)y * (size_t)b.width + (size_t)x;
    if (motion) {
        const float2 m = b.motion[i];
        motion[2 * i] = m.x;
        motion[2 * i + 1] = m.y;
    }
    if (length) length[i] = b.mom[cur][i].z;
}

dim3 rows_grid(int width, int height) { return dim3((unsigned)((width + 63) / 64), (unsigned)((height + 3) / 4)); }

} // namespace

hipError_t launch_temporal_reproject(const TemporalBuffers& b, const TemporalReproject& r, const float* radiance, const float* position,
                                     const float* normal, const float* albedo, const int* ids, hipStream_t stream)
{
    if (b.width <= 0 || b.height <= 0) return hipSuccess;
    hipLaunchKernelGGL(temporal_reproject_kernel, rows_grid(b.width, b.height), dim3(64, 4), 0, stream, b, r, radiance, position, normal, albedo, ids);
    return hipGetLastError();
}

hipError_t launch_temporal_variance(const TemporalBuffers& b, int cur, float variance_history, float inv_sigma_normal, float sigma_plane2,
                                    hipStream_t stream)
{
    if (b.width <= 0 || b.height <= 0) return hipSuccess;
    hipLaunchKernelGGL(temporal_variance_kernel, rows_grid(b.width, b.height), dim3(64, 4), 0, stream, b, cur, variance_history, inv_sigma_normal,
                       sigma_plane2);
    return hipGetLastError();
}

hipError_t launch_temporal_pass(const TemporalBuffers& b, int cur, int src, int pass, float sigma_luminance, float inv_sigma_normal,
                                float sigma_plane2, int same_geometry, float4* feedback, hipStream_t stream)
{
    if (b.width <= 0 || b.height <= 0) return hipSuccess;
    const dim3 grid((unsigned)((b.width + kTile - 1) / kTile), (unsigned)((b.height + kTile - 1) / kTile));
    hipLaunchKernelGGL(temporal_pass_kernel, grid, dim3(kTile * kTile), 0, stream, b, cur, src, 1 << pass, sigma_luminance, inv_sigma_normal,
                       sigma_plane2, same_geometry, feedback);
    return hipGetLastError();
}

hipError_t launch_temporal_history(const TemporalBuffers& b, int cur, float* motion, float* length, hipStream_t stream)
{
    if (b.width <= 0 || b.height <= 0) return hipSuccess;
    hipLaunchKernelGGL(temporal_history_kernel, rows_grid(b.width, b.height), dim3(64, 4), 0, stream, b, cur, motion, length);
    return hipGetLastError();
}

} // namespace ff
